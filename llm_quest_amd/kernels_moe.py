"""Tensor-level launchers of the mixture-of-experts kernels (csrc/moe.hip): router, token-to-expert plan, row dispatch, weighted combine and
their backwards; no autograd here.  Both mixture-of-experts layers use them: the combine is one kernel, and ``combine_fwd`` also takes DeepSeekMoE's
shared experts' output (``kernels_dsmoe.py`` holds only what that layer adds).

Written like ``kernels_mla.py``: every launcher checks shapes / strides / dtypes on the host before a pointer reaches the GPU, allocates its
outputs with torch (or takes them from the caller) and enqueues on torch's current stream.  There is no CPU fallback.

Notation: ``T`` tokens, ``E`` experts, ``k = top_k``, ``d = emb_dim``; ``R = sorted_rows(T, E, k)`` rows of the expert-sorted buffers, a static
bound that does not depend on the routing.  Row operands are bf16 with unit inner stride (row-strided views -- column slices -- allowed).
"""

import torch

from . import _lib as L

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
MAX_EXPERTS, MAX_TOP_K = 128, 8


def row_align():
    """Rows every expert's segment start is a multiple of."""
    return int(L.load().mi355_moe_row_align())


def sorted_rows(T, E, k):
    """Rows of the expert-sorted buffers: every assignment plus the worst-case padding in front of every segment start."""
    return T * k + E * (row_align() - 1)


def check_route(T, E, k):
    if not 1 <= E <= MAX_EXPERTS:
        raise ValueError(f"moe: num_experts must be in 1..{MAX_EXPERTS}, got {E}")
    if not (1 <= k <= MAX_TOP_K and k <= E):
        raise ValueError(f"moe: top_k must be in 1..{MAX_TOP_K} and at most num_experts = {E}, got {k}")
    if T < 0 or T * k + 64 * E >= 2**31:
        raise ValueError(f"moe: tokens * top_k + 64 * num_experts must stay below 2^31, got {T} tokens")


def _rows(t, name, rows, width):
    if t.dtype != BF16 or t.dim() != 2 or t.stride(1) != 1 or tuple(t.shape) != (rows, width):
        raise ValueError(f"moe: {name} must be bf16 [{rows}, {width}] with unit inner stride, got {t.dtype} {tuple(t.shape)} {t.stride()}")
    if width % 8:
        raise ValueError(f"moe: {name}: the row width {width} must be a multiple of 8")
    if rows > 1 and (t.stride(0) < width or t.stride(0) % 8):
        raise ValueError(f"moe: {name} row stride {t.stride(0)} must be a multiple of 8 and at least {width}")
    if t.data_ptr() % 16:
        raise ValueError(f"moe: {name} must be 16-byte aligned")


def _gate_rows(t, name, T, E):
    if t.dtype != BF16 or t.dim() != 2 or t.stride(1) != 1 or tuple(t.shape) != (T, E) or (T > 1 and t.stride(0) < E):
        raise ValueError(f"moe: {name} must be bf16 [{T}, {E}] with unit inner stride, got {t.dtype} {tuple(t.shape)} {t.stride()}")


def _flat(t, name, dtype, shape):
    if t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError(f"moe: {name} must be contiguous {dtype} {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def route_fwd(gate_in, k, replay=False):
    """``gate_in`` bf16 [T, E]: the gate's logits, or with ``replay`` the probabilities to route by.
    Returns (p bf16 [T, E], idx int32 [T, k], w bf16 [T, k], s fp32 [T]); with ``replay`` p is ``gate_in`` itself."""
    L.require_gpu(gate_in)
    if gate_in.dim() != 2:
        raise ValueError("moe: the gate's input must be 2-D (tokens, num_experts)")
    T, E = gate_in.shape
    check_route(T, E, k)
    _gate_rows(gate_in, "gate input", T, E)
    dev = gate_in.device
    p = gate_in if replay else torch.empty((T, E), dtype=BF16, device=dev)
    idx = torch.empty((T, k), dtype=I32, device=dev)
    w = torch.empty((T, k), dtype=BF16, device=dev)
    s = torch.empty((T,), dtype=F32, device=dev)
    L.call("mi355_moe_route_fwd", T, E, k, L.ptr(gate_in), _ld(gate_in), int(replay), None if replay else L.ptr(p), _ld(p), L.ptr(idx), L.ptr(w), L.ptr(s))
    return p, idx, w, s


def route_bwd(dw, w, s, idx, p, counts=None, g=None, aux_loss_coef=0.0, dlogits=None):
    """d(logits) bf16 [T, E] from dw fp32 [T, k]; ``g`` fp32 [1] on the device = dL/d(moe_loss) (None: the loss took no part), then ``counts``."""
    L.require_gpu(dw, w, s, idx, p, counts, g, dlogits)
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
        if counts is None:
            raise ValueError("moe: the load loss's gradient needs the counts")
    if counts is not None:
        _flat(counts, "counts", I32, (E,))
    if dlogits is None:
        dlogits = torch.empty((T, E), dtype=BF16, device=p.device)
    _gate_rows(dlogits, "dlogits", T, E)
    L.call("mi355_moe_route_bwd", T, E, k, L.ptr(dw), L.ptr(w), L.ptr(s), L.ptr(idx), L.ptr(p), _ld(p), L.ptr(counts), L.ptr(g), float(aux_loss_coef),
           L.ptr(dlogits), _ld(dlogits))
    return dlogits


def plan(idx, E, psum=None, aux_loss_coef=0.0):
    """The expert-sorted layout of the assignments ``idx`` int32 [T, k].  Returns (counts [E], offsets [E + 1], slot [T, k], row_token [R], loss):
    ``loss`` fp32 [1] = the load-balancing loss when ``psum`` fp32 [E] (the column sums of the probabilities) is given, else None."""
    L.require_gpu(idx, psum)
    if idx.dim() != 2:
        raise ValueError("moe: idx must be 2-D (tokens, top_k)")
    T, k = idx.shape
    check_route(T, E, k)
    _flat(idx, "idx", I32, (T, k))
    if psum is not None:
        _flat(psum, "psum", F32, (E,))
    dev = idx.device
    R = sorted_rows(T, E, k)
    counts = torch.empty((E,), dtype=I32, device=dev)
    offsets = torch.empty((E + 1,), dtype=I32, device=dev)
    slot = torch.empty((T, k), dtype=I32, device=dev)
    row_token = torch.empty((R,), dtype=I32, device=dev)
    loss = torch.empty((1,), dtype=F32, device=dev) if psum is not None else None
    nbytes = int(L.load().mi355_moe_plan_workspace_bytes(T, E, k))
    ws = torch.empty((max(nbytes // 4, 1),), dtype=I32, device=dev)
    L.call("mi355_moe_plan", T, E, k, L.ptr(idx), L.ptr(counts), L.ptr(offsets), L.ptr(slot), L.ptr(row_token), R, L.ptr(psum), float(aux_loss_coef),
           L.ptr(loss), L.ptr(ws), nbytes)
    return counts, offsets, slot, row_token, loss


def gather_rows(x, row_token, out=None):
    """xs[r] = x[row_token[r]], zeros where row_token is -1."""
    L.require_gpu(x, row_token, out)
    T, d = x.shape
    R = row_token.numel()
    _rows(x, "x", T, d)
    _flat(row_token, "row_token", I32, (R,))
    if out is None:
        out = torch.empty((R, d), dtype=BF16, device=x.device)
    _rows(out, "xs", R, d)
    L.call("mi355_moe_gather_rows", R, T, d, L.ptr(row_token), L.ptr(x), _ld(x), L.ptr(out), _ld(out))
    return out


def combine_fwd(y, slot, w=None, residual=None, out=None, shared=None):
    """out[t] = residual[t] + (shared[t] + sum_j w[t, j] * y[slot[t, j]]), fp32, one rounding; ``w`` None: weights of 1 (the backward of
    ``gather_rows``).  One kernel behind two entry points: ``shared`` (DeepSeekMoE's shared experts' output, which needs ``w``) goes through
    ``mi355_dsmoe_combine_fwd``, everything else through ``mi355_moe_combine_fwd``."""
    if shared is not None and w is None:
        raise ValueError("moe: the combine with a shared operand needs the weights w")
    L.require_gpu(y, slot, w, residual, out, shared)
    R, d = y.shape
    T, k = slot.shape
    _rows(y, "y", R, d)
    _flat(slot, "slot", I32, (T, k))
    if not 1 <= k <= MAX_TOP_K:
        raise ValueError(f"moe: top_k must be in 1..{MAX_TOP_K}, got {k}")
    if w is not None:
        _flat(w, "w", BF16, (T, k))
    if residual is not None:
        _rows(residual, "residual", T, d)
    if out is None:
        out = torch.empty((T, d), dtype=BF16, device=y.device)
    _rows(out, "out", T, d)
    tail = (L.ptr(residual), 0 if residual is None else _ld(residual), L.ptr(out), _ld(out))
    if shared is None:
        L.call("mi355_moe_combine_fwd", T, R, k, d, L.ptr(slot), L.ptr(w), L.ptr(y), _ld(y), *tail)
    else:
        _rows(shared, "shared", T, d)
        L.call("mi355_dsmoe_combine_fwd", T, R, k, d, L.ptr(slot), L.ptr(w), L.ptr(y), _ld(y), L.ptr(shared), _ld(shared), *tail)
    return out


def combine_bwd(dout, row_token, slot, w=None, y=None, dy=None):
    """dy[r] = w(r) * dout[row_token[r]] (zeros on padding rows) and, with ``y``, dw fp32 [T, k] = <dout[t], y[slot[t, j]]>.  Returns (dy, dw)."""
    L.require_gpu(dout, row_token, slot, w, y, dy)
    T, d = dout.shape
    R = row_token.numel()
    k = slot.shape[1]
    _rows(dout, "dout", T, d)
    _flat(row_token, "row_token", I32, (R,))
    _flat(slot, "slot", I32, (T, k))
    if not 1 <= k <= MAX_TOP_K:
        raise ValueError(f"moe: top_k must be in 1..{MAX_TOP_K}, got {k}")
    if w is not None:
        _flat(w, "w", BF16, (T, k))
    dw = None
    if y is not None:
        _rows(y, "y", R, d)
        dw = torch.empty((T, k), dtype=F32, device=dout.device)
    if dy is None:
        dy = torch.empty((R, d), dtype=BF16, device=dout.device)
    _rows(dy, "dy", R, d)
    L.call("mi355_moe_combine_bwd", T, R, k, d, L.ptr(row_token), L.ptr(slot), L.ptr(w), L.ptr(dout), _ld(dout), L.ptr(y), 0 if y is None else _ld(y),
           L.ptr(dy), _ld(dy), L.ptr(dw))
    return dy, dw
