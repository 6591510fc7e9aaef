"""Tensor-level launchers of the label log-probs FROM HIDDEN STATES (csrc/grpo_head.hip): the LM head is walked in vocabulary chunks, so the logits
``[B, S, V]`` never exist -- at most one chunk ``[B S, Vc]`` does, written by a GEMM and read back by a row kernel while it still sits in cache.  No
autograd here (``ops_grpo.HeadLogProbFn``).

Forward, per chunk: ``head_chunk_logits`` (one NT GEMM of the hidden states against rows ``[c0, c1)`` of the weight), then ``mi355_head_lse_chunk``
(online maximum / rescaled sum / the label's logit); ``mi355_head_lse_finish`` closes the state.  Backward, per chunk: the SAME ``head_chunk_logits``
(so the backward sees the very bits the forward saw), ``mi355_head_dlogits_chunk`` in place, then ``dH += dlogits_c W_c`` into one fp32 accumulator and
``dW[c0:c1] (+)= dlogits_c^T H`` into the caller's gradient rows.  That is 4 / 3 of the materialised head's GEMM work, for none of its logits.

Every launcher checks shapes / dtypes / strides on the host first (a refusal reads the same with or without a GPU), then that the operands live on the
device -- there is no CPU fallback.  Neither direction reads anything back to the host: the chunk list depends on shapes alone.  ``h`` is bf16
``[B, S, D]`` contiguous with ``D % 8 == 0``, ``w`` bf16 ``[V, D]`` row-major, ids int64 ``[B, S]``, per-token operands fp32 ``[B, S - 1]``.
"""

import torch

from . import _lib as L
from . import kernels as K0
from .kernels_grpo import BF16, F32, I64, _tok

# The default chunk's logits: half of the 256 MiB Infinity Cache.  Measured at Qwen3-0.6B's head, 4 096 rows (tools/bench_grpo_head.py):
# 64 MiB (8 192 columns) lost 16 % to 128 MiB (16 384 columns); 256 and 512 MiB were 2 .. 3 % slower again and cost their size in scratch.
CHUNK_BYTES = 128 << 20
CHUNK_MIN = 1024


def _ceil8(n):
    return (n + 7) // 8 * 8


def head_chunks(rows, V, vocab_chunk=None):
    """The list of ``(c0, c1)`` that covers ``[0, V)``.  ``vocab_chunk``: a positive multiple of 8, clamped to ``V`` (the last chunk may be ragged, down to
    one column); None: the largest multiple of 128 whose chunk of ``rows`` bf16 rows fits ``CHUNK_BYTES``, but not below ``CHUNK_MIN``."""
    rows, V = int(rows), int(V)
    if rows < 1 or V < 1:
        raise ValueError(f"head_chunks: rows ({rows}) and V ({V}) must be positive")
    if vocab_chunk is None:
        step = max(CHUNK_MIN, CHUNK_BYTES // (rows * 2) // 128 * 128)
    else:
        step = int(vocab_chunk)
        if step != vocab_chunk or step < 1 or step % 8:
            raise ValueError(f"head_chunks: vocab_chunk must be a positive multiple of 8, got {vocab_chunk}")
    step = min(step, V)
    return [(c0, min(c0 + step, V)) for c0 in range(0, V, step)]


def check_head(h, w, ids, what="head_logprob"):
    """The shape / dtype / stride refusals shared by everything that takes (hidden, weight, inputs); returns (B, S, D, V)."""
    if h.dtype != BF16:
        raise TypeError(f"{what}: the hidden states must be bf16 (the HIP path has no other precision), got {h.dtype}")
    if h.dim() != 3:
        raise ValueError(f"{what}: the hidden states must be 3-D (B, S, emb_dim), got {tuple(h.shape)}")
    if w.dtype != BF16:
        raise TypeError(f"{what}: the head's weight must be bf16, got {w.dtype}")
    if w.dim() != 2:
        raise ValueError(f"{what}: the head's weight must be 2-D (vocab_size, emb_dim), got {tuple(w.shape)}")
    B, S, D = h.shape
    V = w.shape[0]
    if ids.dtype != I64 or ids.dim() != 2:
        raise TypeError(f"{what}: the inputs must be int64 [B, S], got {ids.dtype} {tuple(ids.shape)}")
    if tuple(ids.shape) != (B, S):
        raise ValueError(f"{what}: shapes disagree: hidden states {tuple(h.shape)} against inputs {tuple(ids.shape)}")
    if w.shape[1] != D:
        raise ValueError(f"{what}: shapes disagree: hidden states {tuple(h.shape)} against the head's weight {tuple(w.shape)}")
    if B < 1 or S < 1 or V < 1 or D < 1:
        raise ValueError(f"{what}: empty operands: hidden states {tuple(h.shape)}, weight {tuple(w.shape)}")
    if D % 8:
        raise ValueError(f"{what}: emb_dim must be a multiple of 8 (16-byte rows), got {D}")
    if not h.is_contiguous():
        raise ValueError(f"{what}: the hidden states must be contiguous, got strides {tuple(h.stride())}")
    if w.stride(1) != 1 or w.stride(0) < D or w.stride(0) % 8:
        raise ValueError(f"{what}: the head's weight must be row-major with a pitch that is a multiple of 8 elements, got strides {tuple(w.stride())}")
    return B, S, D, V


def check_chunk(chunk, ids, c0, what):
    """A chunk operand of the row kernels: bf16 [B S, Vc] with unit inner stride on rows of a 16-byte pitch, at column offset ``c0``; returns (B, S, Vc)."""
    if chunk.dtype != BF16:
        raise TypeError(f"{what}: the chunk must be bf16, got {chunk.dtype}")
    if chunk.dim() != 2:
        raise ValueError(f"{what}: the chunk must be 2-D (B S, Vc), got {tuple(chunk.shape)}")
    if ids.dtype != I64 or ids.dim() != 2:
        raise TypeError(f"{what}: the inputs must be int64 [B, S], got {ids.dtype} {tuple(ids.shape)}")
    B, S = ids.shape
    rows, Vc = chunk.shape
    if rows != B * S or Vc < 1 or B < 1:
        raise ValueError(f"{what}: shapes disagree: chunk {tuple(chunk.shape)} against inputs {tuple(ids.shape)}")
    if int(c0) < 0 or int(c0) % 8:
        raise ValueError(f"{what}: the chunk's first column must be a non-negative multiple of 8, got {c0}")
    if chunk.stride(1) != 1 or chunk.stride(0) % 8 or chunk.stride(0) < Vc or chunk.data_ptr() % 16:
        raise ValueError(f"{what}: the chunk must have 16-byte rows (unit stride in Vc, row pitch a multiple of 8 elements and >= Vc, 16-byte aligned): "
                         f"strides {tuple(chunk.stride())}")
    return B, S, Vc


def head_lse_chunk(chunk, c0, ids, state, first):
    """One chunk's share of the online log-sum-exp: ``state`` fp32 [3, B, S - 1] = (m, l, label_logit), updated in place (initialised with ``first``)."""
    B, S, Vc = check_chunk(chunk, ids, c0, "head_lse_chunk")
    if state.dtype != F32 or tuple(state.shape) != (3, B, S - 1) or not state.is_contiguous():
        raise ValueError(f"head_lse_chunk: shapes disagree: the state must be contiguous fp32 {(3, B, S - 1)}, got {state.dtype} {tuple(state.shape)}")
    L.require_gpu(chunk, ids, state)
    if S > 1:
        ids = ids if ids.is_contiguous() else ids.contiguous()
        L.call("mi355_head_lse_chunk", B, S, Vc, int(c0), L.ptr(chunk), chunk.stride(0), L.ptr(ids), L.ptr(state[0]), L.ptr(state[1]), L.ptr(state[2]),
               int(bool(first)))
    return state


def head_lse_finish(state):
    """(logp, lse), both fp32 [B, S - 1], from the state all chunks have passed through."""
    if state.dtype != F32 or state.dim() != 3 or state.shape[0] != 3 or not state.is_contiguous():
        raise ValueError(f"head_lse_finish: the state must be contiguous fp32 [3, B, S - 1], got {state.dtype} {tuple(state.shape)}")
    L.require_gpu(state)
    out = torch.empty((2,) + tuple(state.shape[1:]), dtype=F32, device=state.device)
    if out.numel():
        L.call("mi355_head_lse_finish", state[0].numel(), L.ptr(state[0]), L.ptr(state[1]), L.ptr(state[2]), L.ptr(out[0]), L.ptr(out[1]))
    return out[0], out[1]


def head_dlogits_chunk(g, chunk, c0, V, lse, ids, out=None):
    """``out`` (None: ``chunk`` itself, in place) = g (onehot - exp(chunk - lse)) in bf16 for the columns [c0, c0 + Vc) of a vocabulary of ``V``; rows
    S - 1 exact zeros."""
    B, S, Vc = check_chunk(chunk, ids, c0, "head_dlogits_chunk")
    out = chunk if out is None else out
    if tuple(out.shape) != tuple(chunk.shape):
        raise ValueError(f"head_dlogits_chunk: shapes disagree: the output {tuple(out.shape)} against the chunk {tuple(chunk.shape)}")
    check_chunk(out, ids, c0, "head_dlogits_chunk")
    if int(c0) + Vc > int(V):
        raise ValueError(f"head_dlogits_chunk: the chunk [{c0}, {int(c0) + Vc}) does not lie inside the vocabulary ({V})")
    g, lse = _tok(g, "g", B, S - 1), _tok(lse, "lse", B, S - 1)
    L.require_gpu(g, chunk, lse, ids, out)
    if S == 1:
        out.zero_()
        return out
    ids = ids if ids.is_contiguous() else ids.contiguous()
    L.call("mi355_head_dlogits_chunk", B, S, int(V), Vc, int(c0), L.ptr(g), L.ptr(chunk), chunk.stride(0), L.ptr(lse), L.ptr(ids), L.ptr(out), out.stride(0))
    return out


def head_chunk_logits(h2d, w, c0, c1, out):
    """THE place that forms a chunk's logits: ``h2d`` [rows, D] against rows [c0, c1) of ``w`` into the scratch ``out`` bf16 [rows, ceil8(Vc)]; returns
    its first ``Vc`` columns.  Forward and backward both call it, so the backward recomputes the bits the forward saw.  It goes through ``K.gemm`` like
    every NT product: a chunk large enough for the persistent kernel counts against an open GEMM window exactly as the launch it is (``_nt_tick``), and
    nothing here opens or closes one."""
    Vc = int(c1) - int(c0)
    if out.dtype != BF16 or out.dim() != 2 or tuple(out.shape) != (h2d.shape[0], _ceil8(Vc)) or not out.is_contiguous():
        raise ValueError(f"head_chunk_logits: the scratch must be contiguous bf16 {(h2d.shape[0], _ceil8(Vc))}, got {out.dtype} {tuple(out.shape)}")
    return K0.gemm(L.GEMM_NT, h2d, w[c0:c1], out=out[:, :Vc])


def _scratch(rows, chunks, device):
    return torch.empty(rows * max(_ceil8(c1 - c0) for c0, c1 in chunks), dtype=BF16, device=device)


def _chunk_scratch(flat, rows, Vc):
    pitch = _ceil8(Vc)
    return flat[: rows * pitch].view(rows, pitch)


def head_logprob_fwd(h, w, ids, vocab_chunk=None):
    """(logp, lse), both fp32 [B, S - 1]: ``logp[b, s] = (h[b, s] . w[ids[b, s + 1]]) - logsumexp_v(h[b, s] . w[v])`` with the logits rounded to bf16 as
    the head's GEMM rounds them.  All ``B S`` rows go through the GEMM (one pitch keeps it a plain 2-D product).  ``S == 1``: empty results, no launch."""
    B, S, D, V = check_head(h, w, ids, "head_logprob_fwd")
    chunks = head_chunks(B * S, V, vocab_chunk)
    L.require_gpu(h, w, ids)
    if S == 1:
        return torch.empty((B, 0), dtype=F32, device=h.device), torch.empty((B, 0), dtype=F32, device=h.device)
    rows = B * S
    ids = ids if ids.is_contiguous() else ids.contiguous()
    h2d = h.view(rows, D)
    state = torch.empty((3, B, S - 1), dtype=F32, device=h.device)
    flat = _scratch(rows, chunks, h.device)
    for i, (c0, c1) in enumerate(chunks):
        x = head_chunk_logits(h2d, w, c0, c1, _chunk_scratch(flat, rows, c1 - c0))
        head_lse_chunk(x, c0, ids, state, first=i == 0)
    return head_lse_finish(state)


def _dgrad_into(d, wc, acc, first):
    """acc (fp32 [rows, D]) (+)= d wc, in the K-contiguous NT form on the transposed weight chunk where ``K.dgrad`` would take it."""
    res = None if first else acc
    if K0.DGRAD_NT and d.shape[0] >= K0.DGRAD_NT_MIN_ROWS:
        return K0.gemm(L.GEMM_NT, d, K0.transpose(wc), out=acc, residual=res)
    return K0.gemm(L.GEMM_NN, d, wc, out=acc, residual=res)


def head_logprob_bwd(g, h, w, lse, ids, vocab_chunk=None, dw_out=None, dw_accumulate=False):
    """dh bf16 [B, S, D] of ``sum(g * logp)`` for the forward above (``lse`` is its second result, ``vocab_chunk`` any value: the chunks need not be the
    forward's); rows S - 1 exact zeros.  ``dw_out`` ([V, D], bf16 or fp32, row-major): rows [c0, c1) receive ``dlogits_c^T H``, added to what they hold
    with ``dw_accumulate``; None: no weight gradient.  dH is summed over the chunks in ONE fp32 accumulator and rounded to bf16 once.  A ragged last
    chunk (``V % 8 != 0``) goes through zero-padded copies of its weight and gradient rows: the GEMMs take 16-byte rows only."""
    B, S, D, V = check_head(h, w, ids, "head_logprob_bwd")
    T = S - 1
    g, lse = _tok(g, "g", B, T), _tok(lse, "lse", B, T)
    chunks = head_chunks(B * S, V, vocab_chunk)
    if dw_out is not None:
        if dw_out.dtype not in (BF16, F32) or tuple(dw_out.shape) != (V, D):
            raise ValueError(f"head_logprob_bwd: shapes disagree: dw_out must be bf16 or fp32 {(V, D)}, got {dw_out.dtype} {tuple(dw_out.shape)}")
        if dw_out.stride(1) != 1 or dw_out.stride(0) < D or dw_out.stride(0) % 8:
            raise ValueError(f"head_logprob_bwd: dw_out must be row-major with a pitch that is a multiple of 8 elements, got strides {tuple(dw_out.stride())}")
    L.require_gpu(g, h, w, lse, ids, dw_out)
    dev = h.device
    if S == 1:
        if dw_out is not None and not dw_accumulate:
            dw_out.zero_()
        return torch.zeros((B, S, D), dtype=BF16, device=dev)
    rows = B * S
    ids = ids if ids.is_contiguous() else ids.contiguous()
    h2d = h.view(rows, D)
    acc = torch.empty((rows, D), dtype=F32, device=dev)
    flat = _scratch(rows, chunks, dev)
    for i, (c0, c1) in enumerate(chunks):
        Vc = c1 - c0
        sc = _chunk_scratch(flat, rows, Vc)
        d = head_dlogits_chunk(g, head_chunk_logits(h2d, w, c0, c1, sc), c0, V, lse, ids)
        if sc.shape[1] == Vc:
            _dgrad_into(d, w[c0:c1], acc, i == 0)
            if dw_out is not None:
                rows_c = dw_out[c0:c1]
                K0.gemm(L.GEMM_TN, d, h2d, out=rows_c, residual=rows_c if dw_accumulate else None)
            continue
        pitch = sc.shape[1]  # the ragged tail: the same products on operands padded with zero columns / rows
        sc[:, Vc:].zero_()
        wpad = torch.zeros((pitch, D), dtype=BF16, device=dev)
        wpad[:Vc].copy_(w[c0:c1])
        _dgrad_into(sc, wpad, acc, i == 0)
        if dw_out is not None:
            tmp = torch.zeros((pitch, D), dtype=dw_out.dtype, device=dev)
            if dw_accumulate:
                tmp[:Vc].copy_(dw_out[c0:c1])
            K0.gemm(L.GEMM_TN, sc, h2d, out=tmp, residual=tmp if dw_accumulate else None)
            dw_out[c0:c1].copy_(tmp[:Vc])
    return K0.cast(acc, BF16).view(B, S, D)
