"""Tensor-level launchers of the DeepSeekMoE kernels (csrc/deepseek_moe.hip): bias-balanced router, bias update, the shared experts' bias + SiLU
and the fixed-order column sums of the bias gradients; no autograd here.

Written like ``kernels_moe.py``, whose plan / dispatch / combine / combine-backward / router-backward launchers serve this layer too (the combine that
takes the shared experts' output is ``kernels_moe.combine_fwd(..., shared=...)``): every launcher checks shapes / strides / dtypes on the host before a
pointer reaches the GPU and enqueues on torch's current stream.  There is no CPU fallback.
``E`` is the number of ROUTED experts, any value in 1..128.
"""

import torch

from . import _lib as L
from .kernels_moe import _flat, _gate_rows, _ld, _rows, check_route

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32


def _biases(b, E):
    if b.dtype not in (BF16, F32) or b.dim() != 1 or b.numel() != E or not b.is_contiguous():
        raise ValueError(f"dsmoe: biases must be contiguous bf16 or fp32 [{E}], got {b.dtype} {tuple(b.shape)}")


def route_fwd(logits, biases, k, forced_idx=None):
    """``logits`` bf16 [T, E] (row-strided views allowed; columns beyond E are never read), ``biases`` bf16 or fp32 [E].
    Returns (p bf16 [T, E], idx int32 [T, k], w bf16 [T, k], s fp32 [T]); with ``forced_idx`` int32 [T, k] the selection is skipped."""
    L.require_gpu(logits, biases, forced_idx)
    if logits.dim() != 2:
        raise ValueError("dsmoe: the gate's logits must be 2-D (tokens, routed experts)")
    T, E = logits.shape
    check_route(T, E, k)
    _gate_rows(logits, "logits", T, E)
    _biases(biases, E)
    if forced_idx is not None:
        _flat(forced_idx, "forced idx", I32, (T, k))
    dev = logits.device
    p = torch.empty((T, E), dtype=BF16, device=dev)
    idx = torch.empty((T, k), dtype=I32, device=dev)
    w = torch.empty((T, k), dtype=BF16, device=dev)
    s = torch.empty((T,), dtype=F32, device=dev)
    L.call("mi355_dsmoe_route_fwd", T, E, k, L.ptr(logits), _ld(logits), L.ptr(biases), L.dt_code(biases.dtype), L.ptr(forced_idx), L.ptr(p), _ld(p), L.ptr(idx),
           L.ptr(w), L.ptr(s))
    return p, idx, w, s


def bias_update(counts, biases, rate, max_vio=None):
    """biases += rate * sign(mean(counts) - counts) in place; returns max_vio fp32 [1] = (max(counts) - mean) / mean.  No host read."""
    L.require_gpu(counts, biases, max_vio)
    E = biases.numel()
    if not 1 <= E <= 128:
        raise ValueError(f"dsmoe: routed experts must be in 1..128, got {E}")
    _biases(biases, E)
    _flat(counts, "counts", I32, (E,))
    if max_vio is None:
        max_vio = torch.empty((1,), dtype=F32, device=biases.device)
    _flat(max_vio, "max_vio", F32, (1,))
    L.call("mi355_dsmoe_bias_update", E, L.ptr(counts), L.ptr(biases), L.dt_code(biases.dtype), float(rate), L.ptr(max_vio))
    return max_vio


def _bias_row(b, N):
    if b.dtype != BF16 or b.numel() != N or not b.is_contiguous() or b.data_ptr() % 16:
        raise ValueError(f"dsmoe: bias must be contiguous bf16 with {N} elements, 16-byte aligned, got {b.dtype} {tuple(b.shape)}")


def bias_silu_fwd(z, bias):
    """z bf16 [T, N] = x W1 becomes the pre-activation bf16(z + bias) IN PLACE; returns act = bf16(silu(pre))."""
    L.require_gpu(z, bias)
    T, N = z.shape
    _rows(z, "z", T, N)
    _bias_row(bias, N)
    act = torch.empty((T, N), dtype=BF16, device=z.device)
    L.call("mi355_dsmoe_bias_silu_fwd", T, N, L.ptr(z), _ld(z), L.ptr(bias), L.ptr(act), _ld(act))
    return act


def bias_silu_bwd(pre, dact):
    """dpre = bf16(dact * silu'(pre))."""
    L.require_gpu(pre, dact)
    T, N = pre.shape
    _rows(pre, "pre", T, N)
    _rows(dact, "dact", T, N)
    dpre = torch.empty((T, N), dtype=BF16, device=pre.device)
    L.call("mi355_dsmoe_bias_silu_bwd", T, N, L.ptr(pre), _ld(pre), L.ptr(dact), _ld(dact), L.ptr(dpre), _ld(dpre))
    return dpre


def colsum(x):
    """fp32 [N] = the column sums of x bf16 [T, N] (row-strided views allowed) in a FIXED order: per-row-part partials, then ``reduce_rows``.
    (``kernels.colsum`` folds its row blocks with fp32 atomics; the layer's bias gradients must come out the same in every run.)"""
    L.require_gpu(x)
    T, N = x.shape
    _rows(x, "x", T, N)
    n_parts = max(1, min((T + 63) // 64, 128))
    parts = torch.empty((n_parts, N), dtype=F32, device=x.device)
    L.call("mi355_dsmoe_colsum_parts", T, N, L.ptr(x), _ld(x), L.ptr(parts), n_parts)
    return L.reduce_rows(parts)
