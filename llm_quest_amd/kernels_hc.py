"""Tensor-level launchers of the hyper-connection kernels (csrc/hyper_conn.hip); no autograd here.

Written like ``kernels.py``: every launcher checks shapes / strides / dtypes on the host before a pointer reaches the GPU,
allocates its outputs with torch and enqueues on torch's current stream.  There is no CPU fallback.

Notation: ``T`` tokens, ``n`` streams, ``d = emb_dim``; ``X`` is ``[T, n, d]`` bf16 contiguous; the coefficients of the three
connections are fp32 (``Coeffs`` below bundles them for one sub-block).
"""

import os
from collections import namedtuple

import torch

from . import _lib as L

BF16, F32 = torch.bfloat16, torch.float32
HC_FWD_BLOCKS = int(os.environ.get("MI355_HC_FWD_BLOCKS", "2048"))  # max workgroups of the width forward (each walks tokens with this stride)
HC_PARTS = int(os.environ.get("MI355_HC_PARTS", "1024"))  # max workgroups (= rows of partials) of the width backward

# w_norm bf16 [d]; W_res fp32 [n, d]; w_pre / w_post fp32 [d] (or [1, d]); f_* fp32 [1]; b_res fp32 [n, n], b_pre / b_post fp32 [n], or None
Coeffs = namedtuple("Coeffs", "w_norm W_res w_pre w_post f_res f_pre f_post b_res b_pre b_post")
WidthGrads = namedtuple("WidthGrads", "W_res w_pre w_post w_norm f_res f_pre f_post b_res b_pre b_post")


def _streams(x, name, n=None, d=None):
    if x.dim() != 3 or x.dtype != BF16 or not x.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous bf16 [T, n, d] tensor, got {x.dtype} {tuple(x.shape)} strides {x.stride()}")
    if (n is not None and x.shape[1] != n) or (d is not None and x.shape[2] != d):
        raise ValueError(f"{name}: expected [T, {n}, {d}], got {tuple(x.shape)}")


def _single(x, name, T, d):
    if x.dim() != 2 or x.dtype != BF16 or not x.is_contiguous() or tuple(x.shape) != (T, d):
        raise ValueError(f"{name}: expected a contiguous bf16 [{T}, {d}] tensor, got {x.dtype} {tuple(x.shape)} strides {x.stride()}")


def _f32(t, name, numel):
    if t.dtype != F32 or not t.is_contiguous() or t.numel() != numel:
        raise ValueError(f"{name}: expected contiguous fp32 with {numel} elements, got {t.dtype} {tuple(t.shape)}")


def _check_coeffs(c, n, d, biases=True):
    if c.w_norm.dtype != BF16 or not c.w_norm.is_contiguous() or c.w_norm.numel() != d:
        raise ValueError(f"w_norm: expected contiguous bf16 [{d}], got {c.w_norm.dtype} {tuple(c.w_norm.shape)}")
    _f32(c.W_res, "W_res", n * d)
    _f32(c.w_pre, "w_pre", d)
    _f32(c.w_post, "w_post", d)
    for name in ("f_res", "f_pre", "f_post"):
        _f32(getattr(c, name), name, 1)
    if biases:
        for name, numel in (("b_res", n * n), ("b_pre", n), ("b_post", n)):
            if getattr(c, name) is not None:
                _f32(getattr(c, name), name, numel)


def _check_nd(name, n, d, d_max=None):
    if n not in (2, 4):
        raise ValueError(f"{name}: expansion rate n must be 2 or 4, got {n}")
    if d <= 0 or d % 8 != 0 or (d_max is not None and d > d_max):
        raise ValueError(f"{name}: emb_dim must be a positive multiple of 8" + (f", at most {d_max}" if d_max else "") + f", got {d}")


def width_fwd(X, c, eps=1e-6, max_blocks=None):
    """One pass over X -> (R [T,n,d] bf16, P [T,d] bf16, H [T,n+2,n] fp32, TH (tanh values, same shape), rstd [T,n] fp32)."""
    L.require_gpu(X, *[t for t in c if t is not None])
    _streams(X, "X")
    T, n, d = X.shape
    _check_nd("width_fwd", n, d, 4096)
    _check_coeffs(c, n, d)
    dev = X.device
    R = torch.empty_like(X)
    P = torch.empty((T, d), dtype=BF16, device=dev)
    H = torch.empty((T, n + 2, n), dtype=F32, device=dev)
    TH = torch.empty((T, n + 2, n), dtype=F32, device=dev)
    rstd = torch.empty((T, n), dtype=F32, device=dev)
    L.call("mi355_hc_width_fwd", T, n, d, L.ptr(X), L.ptr(c.w_norm), L.ptr(c.W_res), L.ptr(c.w_pre), L.ptr(c.w_post), L.ptr(c.f_res), L.ptr(c.f_pre),
           L.ptr(c.f_post), L.ptr(c.b_res), L.ptr(c.b_pre), L.ptr(c.b_post), L.ptr(R), L.ptr(P), L.ptr(H), L.ptr(TH), L.ptr(rstd), eps,
           max_blocks or HC_FWD_BLOCKS)
    return R, P, H, TH, rstd


def depth_fwd(Y, H, R, out=None):
    """Out[t,i,:] = bf16(bf16(h_post[t,i] * Y[t,:]) + R[t,i,:]) with h_post = H[:, n+1, :]; ``out`` may be ``R`` (in place)."""
    L.require_gpu(Y, H, R, out)
    _streams(R, "R")
    T, n, d = R.shape
    _check_nd("depth_fwd", n, d)
    _single(Y, "Y", T, d)
    _f32(H, "H", T * (n + 2) * n)
    if out is None:
        out = torch.empty_like(R)
    _streams(out, "out", n, d)
    if out.shape[0] != T:
        raise ValueError("depth_fwd: out must have R's shape")
    h_post = H.view(T, n + 2, n)[:, n + 1]
    L.call("mi355_hc_depth_fwd", T, n, d, L.ptr(Y), L.ptr(h_post) if T else None, (n + 2) * n, L.ptr(R), L.ptr(out))
    return out


def depth_bwd(dOut, Y, H):
    """-> (dY [T,d] bf16, dh_post [T,n] fp32); dR is dOut itself."""
    L.require_gpu(dOut, Y, H)
    _streams(dOut, "dOut")
    T, n, d = dOut.shape
    _check_nd("depth_bwd", n, d)
    _single(Y, "Y", T, d)
    _f32(H, "H", T * (n + 2) * n)
    dY = torch.empty_like(Y)
    dh_post = torch.empty((T, n), dtype=F32, device=dOut.device)
    h_post = H.view(T, n + 2, n)[:, n + 1]
    L.call("mi355_hc_depth_bwd", T, n, d, L.ptr(dOut), L.ptr(Y), L.ptr(h_post) if T else None, (n + 2) * n, L.ptr(dY), L.ptr(dh_post))
    return dY, dh_post


def partial_width(n, d):
    return int(L.load().mi355_hc_width_bwd_partial_width(n, d))


def width_bwd(dR, dP, dh_post, X, H, TH, rstd, c, parts=None):
    """-> (dX [T,n,d] bf16, WidthGrads): the parameter gradients are fp32 views of ONE reduced row (sums over tokens: each workgroup leaves a row
    of partials, ``mi355_reduce_rows_f32`` folds them in a fixed order, as ``kernels.rmsnorm_bwd`` does; no atomics, bit-reproducible)."""
    L.require_gpu(dR, dP, dh_post, X, H, TH, rstd, *[t for t in c[:7]])
    _streams(X, "X")
    T, n, d = X.shape
    _check_nd("width_bwd", n, d, 4096)
    if T == 0:
        raise ValueError("width_bwd: no tokens")
    _streams(dR, "dR", n, d)
    if dR.shape[0] != T:
        raise ValueError("width_bwd: dR must have X's shape")
    _single(dP, "dP", T, d)
    _f32(dh_post, "dh_post", T * n)
    _f32(H, "H", T * (n + 2) * n)
    _f32(TH, "TH", T * (n + 2) * n)
    _f32(rstd, "rstd", T * n)
    _check_coeffs(c, n, d, biases=False)
    parts = min(T, parts or HC_PARTS)
    if parts < 1:
        raise ValueError(f"width_bwd: parts must be positive, got {parts}")
    pw = partial_width(n, d)
    dev = X.device
    dX = torch.empty_like(X)
    partial = torch.empty((parts, pw), dtype=F32, device=dev)
    L.call("mi355_hc_width_bwd", T, n, d, L.ptr(dR), L.ptr(dP), L.ptr(dh_post), L.ptr(X), L.ptr(H), L.ptr(TH), L.ptr(rstd), L.ptr(c.w_norm),
           L.ptr(c.W_res), L.ptr(c.w_pre), L.ptr(c.w_post), L.ptr(c.f_res), L.ptr(c.f_pre), L.ptr(c.f_post), L.ptr(dX), L.ptr(partial), parts)
    row = L.reduce_rows(partial)
    o = (n + 3) * d
    g = WidthGrads(
        W_res=row[: n * d].view(n, d), w_pre=row[n * d : (n + 1) * d], w_post=row[(n + 1) * d : (n + 2) * d], w_norm=row[(n + 2) * d : o],
        f_res=row[o : o + 1], f_pre=row[o + 1 : o + 2], f_post=row[o + 2 : o + 3],
        b_res=row[o + 3 : o + 3 + n * n].view(n, n), b_pre=row[o + 3 + n * n : o + 3 + n * n + n], b_post=row[o + 3 + n * n + n : o + 3 + n * n + 2 * n],
    )
    return dX, g


def stream_sum(X):
    """[T, n, d] -> bf16(sum over the streams) [T, d]: fp32 accumulation, one rounding."""
    L.require_gpu(X)
    _streams(X, "X")
    T, n, d = X.shape
    _check_nd("stream_sum", n, d)
    out = torch.empty((T, d), dtype=BF16, device=X.device)
    L.call("mi355_hc_stream_sum", T, n, d, L.ptr(X), L.ptr(out))
    return out


def stream_broadcast(x, n):
    """[T, d] -> [T, n, d], every stream a copy of x."""
    L.require_gpu(x)
    if x.dim() != 2 or x.dtype != BF16 or not x.is_contiguous():
        raise ValueError(f"stream_broadcast: expected a contiguous bf16 [T, d] tensor, got {x.dtype} {tuple(x.shape)}")
    T, d = x.shape
    _check_nd("stream_broadcast", n, d)
    out = torch.empty((T, n, d), dtype=BF16, device=x.device)
    L.call("mi355_hc_stream_broadcast", T, n, d, L.ptr(x), L.ptr(out))
    return out
