"""Tensor-level launchers of the Gemma3 kernels (windowed attention: csrc/attention_band.hip; row kernels: csrc/gemma3.hip); no autograd here.

Written like ``kernels.py`` / ``kernels_hc.py``: every launcher checks shapes / strides / dtypes on the host before a pointer reaches the
GPU, allocates its outputs with torch and enqueues on torch's current stream.  There is no CPU fallback.

Notation: ``T = B * S`` tokens; attention operands are token-major ``[T, heads * D]`` bf16 with unit inner stride (row-strided views
allowed); ``W`` is the window: key j is visible to query i iff ``i - W < j <= i``.
"""

import torch

from . import _lib as L

BF16, F32 = torch.bfloat16, torch.float32
G3_PARTS = 512  # max workgroups (= rows of partials) of the backwards that reduce parameter gradients
HEAD_DIMS = (32, 64, 128)
RMS_EPS, LN_EPS = 1e-6, 1e-5


# ---- host checks of the banded attention family (csrc/attention_band.hip): kernels_mimo.py's sink launchers use them too.  ``who`` is the family
# label of the error texts ("swa attention" / "sink attention"); D is the q / k head dim, DV the v / o head dim.
def _attn_operand(who, t, name, tokens, width):
    if t.dtype != BF16 or t.dim() != 2 or t.stride(1) != 1 or t.shape[0] != tokens or t.shape[1] != width:
        raise ValueError(f"{who}: {name} must be bf16 [tokens={tokens}, {width}] with unit inner stride, got {t.dtype} {tuple(t.shape)} {t.stride()}")
    if tokens > 1 and (t.stride(0) < width or t.stride(0) % 8):
        raise ValueError(f"{who}: {name} row stride {t.stride(0)} must be a multiple of 8 and at least {width}")
    if t.data_ptr() % 16:
        raise ValueError(f"{who}: {name} must be 16-byte aligned")


def _check_attn(who, B, S, Hq, Hkv, W, dims_error):
    """``dims_error``: None, or what to say of head dims that the family does not build (reported in its old place among the checks)."""
    if B < 0 or S < 0:
        raise ValueError(f"{who}: negative batch or sequence length ({B}, {S})")
    if W < 1:
        raise ValueError(f"{who}: window must be at least 1, got {W}")
    if dims_error:
        raise ValueError(f"{who}: {dims_error}")
    if Hq <= 0 or Hkv <= 0 or Hq % Hkv:
        raise ValueError(f"{who}: query heads ({Hq}) must be a multiple of kv heads ({Hkv})")


def _fwd_operands(who, q, k, v, B, S, Hq, Hkv, D, DV):
    _attn_operand(who, q, "q", B * S, Hq * D)
    _attn_operand(who, k, "k", B * S, Hkv * D)
    _attn_operand(who, v, "v", B * S, Hkv * DV)


def _bwd_operands(who, q, k, v, o, do, lse, dq, dk, dv, B, S, Hq, Hkv, D, DV):
    """Checks the backward's operands; dq / dk / dv that are None are allocated.  Returns (dq, dk, dv)."""
    dev = q.device
    dq = torch.empty((B * S, Hq * D), dtype=BF16, device=dev) if dq is None else dq
    dk = torch.empty((B * S, Hkv * D), dtype=BF16, device=dev) if dk is None else dk
    dv = torch.empty((B * S, Hkv * DV), dtype=BF16, device=dev) if dv is None else dv
    for t, n, w in ((q, "q", Hq * D), (k, "k", Hkv * D), (v, "v", Hkv * DV), (o, "o", Hq * DV), (do, "do", Hq * DV), (dq, "dq", Hq * D), (dk, "dk", Hkv * D),
                    (dv, "dv", Hkv * DV)):
        _attn_operand(who, t, n, B * S, w)
    if not (lse.dtype == F32 and lse.is_contiguous() and tuple(lse.shape) == (B, Hq, S)):
        raise ValueError(f"{who}: lse must be contiguous fp32 [B,Hq,S]")
    return dq, dk, dv


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def _dims_error(D):
    return None if D in HEAD_DIMS else f"head_dim {D} not built {HEAD_DIMS}"


def swa_attn_fwd(q, k, v, B, S, Hq, Hkv, D, W, scale=None):
    """Sliding-window causal attention.  Returns (o [B*S, Hq*D] bf16, lse fp32 [B, Hq, S])."""
    L.require_gpu(q, k, v)
    _check_attn("swa attention", B, S, Hq, Hkv, W, _dims_error(D))
    _fwd_operands("swa attention", q, k, v, B, S, Hq, Hkv, D, D)
    o = torch.empty((B * S, Hq * D), dtype=BF16, device=q.device)
    lse = torch.empty((B, Hq, S), dtype=F32, device=q.device)
    scale = D ** -0.5 if scale is None else scale
    L.call("mi355_swa_attn_fwd", B, S, Hq, Hkv, D, min(int(W), 2**31 - 1), L.ptr(q), _ld(q), L.ptr(k), _ld(k), L.ptr(v), _ld(v), L.ptr(o), Hq * D, L.ptr(lse), scale)
    return o, lse


def swa_attn_bwd(q, k, v, o, do, lse, B, S, Hq, Hkv, D, W, dq=None, dk=None, dv=None, scale=None):
    """dq / dk / dv: caller-provided (possibly row-strided) destinations, or new tensors.  Returns (dq, dk, dv)."""
    L.require_gpu(q, k, v, o, do, lse, dq, dk, dv)
    _check_attn("swa attention", B, S, Hq, Hkv, W, _dims_error(D))
    dq, dk, dv = _bwd_operands("swa attention", q, k, v, o, do, lse, dq, dk, dv, B, S, Hq, Hkv, D, D)
    delta = torch.empty_like(lse)
    scale = D ** -0.5 if scale is None else scale
    L.call("mi355_swa_attn_bwd", B, S, Hq, Hkv, D, min(int(W), 2**31 - 1), L.ptr(q), _ld(q), L.ptr(k), _ld(k), L.ptr(v), _ld(v), L.ptr(o), _ld(o), L.ptr(do), _ld(do),
           L.ptr(lse), L.ptr(delta), L.ptr(dq), _ld(dq), L.ptr(dk), _ld(dk), L.ptr(dv), _ld(dv), scale)
    return dq, dk, dv


def _rows(t, name, shape=None):
    if t.dim() != 2 or t.dtype != BF16 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"{name}: expected a contiguous bf16 {list(shape) if shape is not None else '[rows, width]'} tensor, got {t.dtype} {tuple(t.shape)} strides {t.stride()}")
    if t.data_ptr() % 16:
        raise ValueError(f"{name}: must be 16-byte aligned")


def _vec(t, name, n):
    if t.dtype != BF16 or not t.is_contiguous() or t.numel() != n:
        raise ValueError(f"{name}: expected contiguous bf16 with {n} elements, got {t.dtype} {tuple(t.shape)}")
    if t.data_ptr() % 16:
        raise ValueError(f"{name}: must be 16-byte aligned")


def _parts(rows, parts):
    parts = min(G3_PARTS, (rows + 3) // 4) if parts is None else parts
    if parts < 1:
        raise ValueError(f"parts must be positive, got {parts}")
    return parts


def rmsnorm_fwd(x, scale, residual=None, eps=RMS_EPS):
    """bf16(scale * x / (sqrt(mean(x^2)) + eps) [+ residual]) over rows of x [rows, width]."""
    L.require_gpu(x, scale, residual)
    _rows(x, "g3 rmsnorm_fwd: x")
    rows, width = x.shape
    if width <= 0 or width % 8:
        raise ValueError(f"g3 rmsnorm_fwd: width must be a positive multiple of 8, got {width}")
    _vec(scale, "g3 rmsnorm_fwd: scale", width)
    if residual is not None:
        _rows(residual, "g3 rmsnorm_fwd: residual", x.shape)
    y = torch.empty_like(x)
    L.call("mi355_g3_rmsnorm_fwd", rows, width, L.ptr(x), L.ptr(residual), L.ptr(scale), L.ptr(y), eps)
    return y


def rmsnorm_bwd(x, scale, dy, dres=None, eps=RMS_EPS, parts=None):
    """-> (dx [+ dres] bf16, dscale fp32 [width]); the column sums go through per-workgroup partial rows and mi355_reduce_rows_f32."""
    L.require_gpu(x, scale, dy, dres)
    _rows(x, "g3 rmsnorm_bwd: x")
    rows, width = x.shape
    if rows == 0:
        raise ValueError("g3 rmsnorm_bwd: no rows")
    if width <= 0 or width % 8 or width > 4096:
        raise ValueError(f"g3 rmsnorm_bwd: width must be a positive multiple of 8, at most 4096, got {width}")
    _vec(scale, "g3 rmsnorm_bwd: scale", width)
    _rows(dy, "g3 rmsnorm_bwd: dy", x.shape)
    if dres is not None:
        _rows(dres, "g3 rmsnorm_bwd: dres", x.shape)
    parts = _parts(rows, parts)
    dx = torch.empty_like(x)
    part = torch.empty((parts, width), dtype=F32, device=x.device)
    L.call("mi355_g3_rmsnorm_bwd", rows, width, L.ptr(x), L.ptr(scale), L.ptr(dy), L.ptr(dres), L.ptr(dx), L.ptr(part), parts, eps)
    return dx, L.reduce_rows(part)


def _check_rope_ln(name, x, S, Hq, Hkv, D, cos, sin, params):
    if D not in HEAD_DIMS:
        raise ValueError(f"{name}: head_dim {D} not built {HEAD_DIMS}")
    if Hq < 0 or Hkv < 0 or Hq + Hkv == 0 or S <= 0:
        raise ValueError(f"{name}: bad head counts / sequence length ({Hq}, {Hkv}, {S})")
    width = (Hq + Hkv) * D
    if x.dim() != 2 or x.dtype != BF16 or x.stride(1) != 1 or x.shape[1] < width or (x.shape[0] > 1 and x.stride(0) < width):
        raise ValueError(f"{name}: expected bf16 [tokens, >= {width}] with unit inner stride, got {x.dtype} {tuple(x.shape)} {x.stride()}")
    if x.shape[0] % S:
        raise ValueError(f"{name}: {x.shape[0]} tokens are no multiple of the sequence length {S}")
    for t, n in ((cos, "cos"), (sin, "sin")):
        if t.dtype != F32 or not t.is_contiguous() or t.dim() != 2 or t.shape[1] != D or t.shape[0] < S:
            raise ValueError(f"{name}: {n} must be contiguous fp32 [>= {S}, {D}], got {t.dtype} {tuple(t.shape)}")
    for t, n in zip(params, ("q_scale", "q_shift", "k_scale", "k_shift")):
        _vec(t, f"{name}: {n}", D)


def rope_ln_fwd(x, S, Hq, Hkv, D, cos, sin, q_scale, q_shift, k_scale, k_shift, eps=LN_EPS):
    """RoPE then per-head LayerNorm on the q and k heads of x [T, >= (Hq+Hkv)*D] (q heads first; further columns, the v heads of a fused
    projection, are not touched).  Returns y [T, (Hq+Hkv)*D] bf16."""
    params = (q_scale, q_shift, k_scale, k_shift)
    L.require_gpu(x, cos, sin, *params)
    _check_rope_ln("g3 rope_ln_fwd", x, S, Hq, Hkv, D, cos, sin, params)
    T, width = x.shape[0], (Hq + Hkv) * D
    y = torch.empty((T, width), dtype=BF16, device=x.device)
    L.call("mi355_g3_rope_ln_fwd", T, S, Hq, Hkv, D, L.ptr(x), max(x.stride(0), width), L.ptr(cos), L.ptr(sin), cos.shape[0], *[L.ptr(p) for p in params], L.ptr(y), width, eps)
    return y


def rope_ln_bwd(x, dy, S, Hq, Hkv, D, cos, sin, q_scale, q_shift, k_scale, k_shift, dx=None, eps=LN_EPS, parts=None):
    """-> (dx, dq_scale, dq_shift, dk_scale, dk_shift): dx bf16 like the q / k columns of x (``dx`` may be a row-strided destination, the
    gradient of a fused projection), the four parameter gradients fp32 [D] views of one reduced row."""
    params = (q_scale, q_shift, k_scale, k_shift)
    L.require_gpu(x, dy, cos, sin, dx, *params)
    _check_rope_ln("g3 rope_ln_bwd", x, S, Hq, Hkv, D, cos, sin, params)
    T, width = x.shape[0], (Hq + Hkv) * D
    if T == 0:
        raise ValueError("g3 rope_ln_bwd: no tokens")
    if dx is None:
        dx = torch.empty((T, width), dtype=BF16, device=x.device)
    for t, n in ((dy, "dy"), (dx, "dx")):
        if t.dim() != 2 or t.dtype != BF16 or t.stride(1) != 1 or t.shape[0] != T or t.shape[1] < width or (T > 1 and t.stride(0) < width):
            raise ValueError(f"g3 rope_ln_bwd: {n} must be bf16 [{T}, >= {width}] with unit inner stride, got {t.dtype} {tuple(t.shape)} {t.stride()}")
    parts = _parts(T * (Hq + Hkv) * D // 128 + 1, parts)
    part = torch.empty((parts, 4 * D), dtype=F32, device=x.device)
    L.call("mi355_g3_rope_ln_bwd", T, S, Hq, Hkv, D, L.ptr(x), max(x.stride(0), width), L.ptr(cos), L.ptr(sin), cos.shape[0], *[L.ptr(p) for p in params],
           L.ptr(dy), max(dy.stride(0), width), L.ptr(dx), max(dx.stride(0), width), L.ptr(part), parts, eps)
    row = L.reduce_rows(part)
    return dx, row[:D], row[D : 2 * D], row[2 * D : 3 * D], row[3 * D :]


def geglu_fwd(gu, F):
    """gu [T, 2F] = [lin1 | lin_gate] -> a = lin1 * gelu_erf(lin_gate), bf16 [T, F]."""
    L.require_gpu(gu)
    if F <= 0 or F % 8:
        raise ValueError(f"geglu_fwd: F must be a positive multiple of 8, got {F}")
    _rows(gu, "geglu_fwd: gu", (gu.shape[0], 2 * F))
    a = torch.empty((gu.shape[0], F), dtype=BF16, device=gu.device)
    L.call("mi355_geglu_fwd", gu.shape[0], F, L.ptr(gu), L.ptr(a))
    return a


def geglu_bwd(gu, da, F):
    L.require_gpu(gu, da)
    if F <= 0 or F % 8:
        raise ValueError(f"geglu_bwd: F must be a positive multiple of 8, got {F}")
    _rows(gu, "geglu_bwd: gu", (gu.shape[0], 2 * F))
    _rows(da, "geglu_bwd: da", (gu.shape[0], F))
    dgu = torch.empty_like(gu)
    L.call("mi355_geglu_bwd", gu.shape[0], F, L.ptr(gu), L.ptr(da), L.ptr(dgu))
    return dgu
