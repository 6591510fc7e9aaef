"""Tensor-level launchers of the classic-MoE kernels (csrc/classic_moe.hip): the softmax router that also leaves the tokens' logsumexp, its backward
with the z term, the layer's loss, the per-expert bias (+ erf GELU) on the expert-sorted buffer and the biases' gradients; no autograd here.

Written like ``kernels_latmoe.py`` and on ``kernels_moe.py``'s checks: every launcher checks shapes / strides / dtypes on the host before a pointer
reaches the GPU and enqueues on torch's current stream.  There is no CPU fallback.  Plan, dispatch and combine are ``kernels_moe.py``'s; the GELU
backward is ``kernels.gelu_bwd`` on the contiguous sorted buffer (``gelu_bwd`` below only checks the rows).
``counts`` / ``offsets`` are ``kernels_moe.plan``'s device tensors and are never read by the host.
"""

import torch

from . import _lib as L
from . import kernels as K
from .kernels import _check_seg_table, _check_stack
from .kernels_moe import _flat, _gate_rows, _ld, _rows, check_route

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
MAX_PARTS = 64  # csrc/classic_moe.hip: the row parts of a segment's column sums


def route_fwd(logits, k, forced_idx=None, p=None):
    """``logits`` bf16 [T, E] (row-strided views allowed; columns beyond E are never read).  Returns (p bf16 [T, E] = bf16(softmax), idx int32 [T, k],
    w bf16 [T, k], s fp32 [T], lse fp32 [T] = bf16(logsumexp)); with ``forced_idx`` int32 [T, k] the selection is skipped.  ``p``: a destination."""
    L.require_gpu(logits, forced_idx, p)
    if logits.dim() != 2:
        raise ValueError("cmoe: the gate's logits must be 2-D (tokens, num_experts)")
    T, E = logits.shape
    check_route(T, E, k)
    _gate_rows(logits, "logits", T, E)
    if forced_idx is not None:
        _flat(forced_idx, "forced idx", I32, (T, k))
    dev = logits.device
    if p is None:
        p = torch.empty((T, E), dtype=BF16, device=dev)
    _gate_rows(p, "p", T, E)
    idx = torch.empty((T, k), dtype=I32, device=dev)
    w = torch.empty((T, k), dtype=BF16, device=dev)
    s = torch.empty((T,), dtype=F32, device=dev)
    lse = torch.empty((T,), dtype=F32, device=dev)
    L.call("mi355_cmoe_route_fwd", T, E, k, L.ptr(logits), _ld(logits), L.ptr(forced_idx), L.ptr(p), _ld(p), L.ptr(idx), L.ptr(w), L.ptr(s), L.ptr(lse))
    return p, idx, w, s, lse


def route_bwd(dw, w, s, idx, p, counts=None, g=None, load_coeff=0.0, z_router_coeff=0.0, lse=None, dlogits=None):
    """d(logits) bf16 [T, E] from dw fp32 [T, k]; ``g`` fp32 [1] on the device = dL/d(moe_loss) (None: the loss took no part), then ``counts`` and ``lse``."""
    L.require_gpu(dw, w, s, idx, p, counts, g, lse, dlogits)
    if idx.dim() != 2 or p.dim() != 2:
        raise ValueError("cmoe: idx must be 2-D (tokens, top_k) and p 2-D (tokens, num_experts)")
    T, k = idx.shape
    E = p.shape[1]
    check_route(T, E, k)
    _flat(dw, "dw", F32, (T, k))
    _flat(w, "w", BF16, (T, k))
    _flat(s, "s", F32, (T,))
    _flat(idx, "idx", I32, (T, k))
    _gate_rows(p, "p", T, E)
    if g is not None:
        _flat(g, "g", F32, (1,))
        if counts is None or lse is None:
            raise ValueError("cmoe: the loss's gradient needs the counts and lse")
    if counts is not None:
        _flat(counts, "counts", I32, (E,))
    if lse is not None:
        _flat(lse, "lse", F32, (T,))
    if dlogits is None:
        dlogits = torch.empty((T, E), dtype=BF16, device=p.device)
    _gate_rows(dlogits, "dlogits", T, E)
    L.call("mi355_cmoe_route_bwd", T, E, k, L.ptr(dw), L.ptr(w), L.ptr(s), L.ptr(idx), L.ptr(p), _ld(p), L.ptr(counts), L.ptr(g), float(load_coeff),
           float(z_router_coeff), L.ptr(lse), L.ptr(dlogits), _ld(dlogits))
    return dlogits


def loss(lse, z_router_coeff, load_loss=None):
    """fp32 [1] = bf16(bf16(z_router_coeff * bf16(mean_t bf16(lse_t^2))) + load_loss): one workgroup, one summation order.  ``load_loss`` fp32 [1]:
    what ``kernels_moe.plan`` returned, or None."""
    L.require_gpu(lse, load_loss)
    T = lse.numel()
    if T < 1:
        raise ValueError("cmoe: the loss needs at least one token")
    _flat(lse, "lse", F32, (T,))
    if load_loss is not None:
        _flat(load_loss, "load loss", F32, (1,))
    out = torch.empty((1,), dtype=F32, device=lse.device)
    L.call("mi355_cmoe_loss", T, L.ptr(lse), float(z_router_coeff), L.ptr(load_loss), L.ptr(out))
    return out


def _bias_stack(b, name, E, N, dtypes=(BF16,)):
    """[E, 1, N] (``kernels.expert_stack`` over the experts' bias vectors) -> the distance between two experts in elements."""
    _check_stack(b, f"cmoe: {name}", dtypes)
    if tuple(b.shape) != (E, 1, N):
        raise ValueError(f"cmoe: {name} must be the experts' stack [{E}, 1, {N}], got {tuple(b.shape)}")
    return b.stride(0) if E > 1 else max(b.stride(0), N)


def bias_act_fwd(z, bias, counts, offsets, gelu, pre=None, act=None):
    """The experts' bias on the sorted rows ``z`` bf16 [R, N]: row r gets ``bias[e(r)]`` ([E, 1, N], ``kernels.expert_stack``), the sum goes to ``pre``
    (None: in place).  ``gelu``: also returns act = bf16(gelu_erf(pre)), else None.  Padding rows are neither read nor written."""
    L.require_gpu(z, bias, counts, offsets, pre, act)
    if z.dim() != 2 or bias.dim() != 3:
        raise ValueError("cmoe: z must be 2-D [R, N] and the biases a stack [E, 1, N]")
    R, N = z.shape
    E = bias.shape[0]
    _rows(z, "z", R, N)
    stride = _bias_stack(bias, "bias", E, N)
    _check_seg_table(counts, offsets, E)
    if pre is not None:
        _rows(pre, "pre", R, N)
    if gelu:
        if act is None:
            act = torch.empty((R, N), dtype=BF16, device=z.device)
        _rows(act, "act", R, N)
    L.call("mi355_cmoe_bias_act_fwd", R, N, E, L.ptr(counts), L.ptr(offsets), L.ptr(z), _ld(z), L.ptr(bias), stride, L.ptr(pre), 0 if pre is None else _ld(pre),
           L.ptr(act) if gelu else None, _ld(act) if gelu else 0, 1 if gelu else 0)
    return act if gelu else None


def gelu_bwd(pre, dact):
    """dpre = bf16(dact * gelu_erf'(pre)) on the contiguous sorted buffers [R, N]: ``mi355_gelu_bwd`` (row-independent, so padding rows touch nothing else)."""
    if pre.dim() != 2 or pre.dtype != BF16 or not pre.is_contiguous() or pre.shape[1] % 8:
        raise ValueError(f"cmoe: pre must be contiguous bf16 [R, N] with N % 8 == 0, got {pre.dtype} {tuple(pre.shape)} {pre.stride()}")
    return K.gelu_bwd(pre, dact)


def segment_colsum(x, counts, offsets, out, accumulate=False):
    """out[e, 0, :] (+)= the column sums of expert e's row segment of ``x`` bf16 [R, N]; ``out`` [E, 1, N] bf16 or fp32 (``kernels.expert_stack`` over the
    bias gradients, or a plain tensor).  fp32 sums in a fixed order; an expert without a row gets exactly zero (accumulating: is not touched)."""
    L.require_gpu(x, counts, offsets, out)
    if x.dim() != 2 or out.dim() != 3:
        raise ValueError("cmoe: x must be 2-D [R, N] and out a stack [E, 1, N]")
    R, N = x.shape
    E = out.shape[0]
    _rows(x, "x", R, N)
    stride = _bias_stack(out, "out", E, N, (BF16, F32))
    _check_seg_table(counts, offsets, E)
    n_parts = max(1, min(MAX_PARTS, 1024 // (E * ((N + 511) // 512)), (R + 63) // 64))
    parts = torch.empty((E, n_parts, N), dtype=F32, device=x.device)
    L.call("mi355_cmoe_segment_colsum", R, N, E, L.ptr(counts), L.ptr(offsets), L.ptr(x), _ld(x), L.ptr(parts), n_parts, L.ptr(out), stride, L.dt_code(out.dtype),
           int(accumulate))
    return out
