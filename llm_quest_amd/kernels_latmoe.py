"""Tensor-level launchers of the LatentMoE kernels (csrc/latent_moe.hip): the sigmoid router with balancing biases and a scaling factor, its backward,
and the squared-ReLU gated activation, forward and backward; no autograd here.

Written like ``kernels_dsmoe.py``: every launcher checks shapes / strides / dtypes on the host before a pointer reaches the GPU and enqueues on torch's
current stream.  There is no CPU fallback.  Plan, dispatch and combine are ``kernels_moe.py``'s, the bias update ``kernels_dsmoe.bias_update``.
``E`` is the number of routed experts, any value in 1..128.
"""

import torch

from . import _lib as L
from .kernels_dsmoe import _biases
from .kernels_moe import _flat, _gate_rows, _ld, _rows, check_route

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32


def route_fwd(logits, biases, k, scaling, forced_idx=None):
    """``logits`` bf16 [T, E] (row-strided views allowed; columns beyond E are never read), ``biases`` bf16 or fp32 [E].
    Returns (p bf16 [T, E] = bf16(sigmoid), idx int32 [T, k], w bf16 [T, k] = bf16(bf16(v / s) * scaling), s fp32 [T]); with ``forced_idx``
    int32 [T, k] the selection is skipped."""
    L.require_gpu(logits, biases, forced_idx)
    if logits.dim() != 2:
        raise ValueError("latmoe: the gate's logits must be 2-D (tokens, routed experts)")
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
    L.call("mi355_latmoe_route_fwd", T, E, k, L.ptr(logits), _ld(logits), L.ptr(biases), L.dt_code(biases.dtype), L.ptr(forced_idx), float(scaling), L.ptr(p), _ld(p),
           L.ptr(idx), L.ptr(w), L.ptr(s))
    return p, idx, w, s


def route_bwd(dw, s, idx, p, scaling, dlogits=None):
    """d(logits) bf16 [T, E] from dw fp32 [T, k]: non-zero at the selected experts only.  ``dlogits`` may be a column slice of a wider buffer."""
    L.require_gpu(dw, s, idx, p, dlogits)
    if idx.dim() != 2 or p.dim() != 2:
        raise ValueError("latmoe: idx must be 2-D (tokens, top_k) and p 2-D (tokens, routed experts)")
    T, k = idx.shape
    E = p.shape[1]
    check_route(T, E, k)
    _flat(dw, "dw", F32, (T, k))
    _flat(s, "s", F32, (T,))
    _flat(idx, "idx", I32, (T, k))
    _gate_rows(p, "p", T, E)
    if dlogits is None:
        dlogits = torch.empty((T, E), dtype=BF16, device=p.device)
    _gate_rows(dlogits, "dlogits", T, E)
    L.call("mi355_latmoe_route_bwd", T, E, k, L.ptr(dw), L.ptr(s), L.ptr(idx), L.ptr(p), _ld(p), float(scaling), L.ptr(dlogits), _ld(dlogits))
    return dlogits


def _pair(gu, F_):
    if gu.dim() != 2 or F_ <= 0 or gu.shape[1] != 2 * F_:
        raise ValueError(f"latmoe: the fused pair [u | g] must be 2-D with 2 * {F_} columns, got {tuple(gu.shape)}")
    _rows(gu, "gu", gu.shape[0], 2 * F_)
    if F_ % 8:
        raise ValueError(f"latmoe: the hidden size {F_} must be a multiple of 8")
    return gu.shape[0]


def relu2_glu_fwd(gu, F_, out=None):
    """a bf16 [R, F] = bf16(u * bf16(relu(g)^2)) from gu bf16 [R, 2F] = [u | g] (row-strided views allowed)."""
    L.require_gpu(gu, out)
    R = _pair(gu, F_)
    if out is None:
        out = torch.empty((R, F_), dtype=BF16, device=gu.device)
    _rows(out, "a", R, F_)
    L.call("mi355_latmoe_relu2_glu_fwd", R, F_, L.ptr(gu), _ld(gu), L.ptr(out), _ld(out))
    return out


def relu2_glu_bwd(gu, da, F_, out=None):
    """dgu bf16 [R, 2F] = [da * q | da * u * 2 relu(g)] from the forward's gu and da bf16 [R, F]; the g half is exactly zero where g <= 0."""
    L.require_gpu(gu, da, out)
    R = _pair(gu, F_)
    _rows(da, "da", R, F_)
    if out is None:
        out = torch.empty((R, 2 * F_), dtype=BF16, device=gu.device)
    _rows(out, "dgu", R, 2 * F_)
    L.call("mi355_latmoe_relu2_glu_bwd", R, F_, L.ptr(gu), _ld(gu), L.ptr(da), _ld(da), L.ptr(out), _ld(out))
    return out
