"""Autograd layer of the MiMo-V2-Flash path (``xiaomi/``) over the kernels of ``kernels_mimo.py``, the DeepSeekMoE layer of ``ops_dsmoe.py`` and the
existing GEMMs, norms and SwiGLU kernels.

Same design as ``ops.py`` / ``ops_g3.py`` / ``ops_mla.py``: activations are token-major 2-D bf16 tensors, a transformer block is ONE autograd node
with a hand-written backward, weight gradients are written by the wgrad GEMMs straight into the block's gradient arena, and the vector gradients
(norm weights, the sink) are reduced deterministically and added into it.

Block forward (x [M, d]; Hq query heads of D features, Hkv kv heads, values DV wide):
    h1 = rmsnorm(x) -> qkv = h1 [Wq | Wk | Wv]^T  [M, (Hq + Hkv) D + Hkv DV]
    per-head RMSNorm + partial RoPE on the q / k columns -> attention with the layer's window and sink (SWA) or causal without one (GA)
    x2 = ctx Wo^T + x -> h2 = rmsnorm(x2) -> x3 = FFN(h2) + x2 (dense SwiGLU on the fused gate-up kernels) or DeepSeekMoE(h2) + x2 (on the combine)
The dense causal / band mask buffers of the reference are never read: the window is a number.
"""

import torch

from . import _lib as L
from . import kernels as K
from . import kernels_mimo as KM
from . import ops_dsmoe, ops_mla
from .ops import _flush_wgrads, _vecgrad, _wgrad, arena_for
from .ops_g3 import _add_vecgrad, _check_activation, _flat, _param_list, check_bf16  # noqa: F401  (re-exported for the modules)

BF16, F32 = torch.bfloat16, torch.float32


class Runtime:
    """Per-forward constants of the layers of one kind (SWA or GA): batch, sequence length, window (S for a GA layer), fp32 RoPE tables [>= S, R]."""

    __slots__ = ("B", "S", "W", "cos", "sin")

    def __init__(self, B, S, W, cos, sin):
        self.B, self.S, self.W, self.cos, self.sin = B, S, W, cos, sin


def _tables_f32(owner, cos, sin):
    """The RoPE tables as the kernels take them, fp32 and contiguous (``.to(torch.bfloat16)`` casts the buffers along with the parameters; the
    kernels multiply by bf16-rounded cos / sin anyway, so casting them back up is lossless).  Cached on ``owner`` per storage: a model holds two
    table sets, and an MTP step passes a row slice of one of them.  An entry keeps its source tensors alive, so its addresses cannot pass to others."""
    if cos.dtype == F32 and sin.dtype == F32 and cos.is_contiguous() and sin.is_contiguous():
        return cos, sin
    cache = getattr(owner, "_rope_f32", None)
    if cache is None:
        cache = {}
        object.__setattr__(owner, "_rope_f32", cache)
    key = (cos.data_ptr(), sin.data_ptr(), cos.dtype, tuple(cos.shape), cos._version, sin._version)
    if key not in cache:
        if len(cache) >= 8:
            cache.clear()
        cache[key] = (K.cast(cos.contiguous(), F32), K.cast(sin.contiguous(), F32), cos, sin)
    return cache[key][:2]


def make_runtime(owner, B, S, window, cos, sin, context_length=None):
    """``window``: the layer's window size, or None for a global-attention layer (W = S)."""
    limit = cos.shape[0] if context_length is None else context_length
    if S > limit:
        raise ValueError(f"sequence length {S} exceeds context_length {limit}")
    if window is not None and window < 1:
        raise ValueError(f"window_size must be at least 1, got {window}")
    L.require_gpu(cos, sin)
    cos, sin = _tables_f32(owner, cos, sin)
    return Runtime(B, S, max(S, 1) if window is None else int(window), cos, sin)


def refuse_attn_mask(attn_mask, what):
    if attn_mask is not None:
        raise NotImplementedError(f"{what}: attn_mask (a padding mask) is not supported by the sink attention kernels; pass attn_mask=None "
                                  f"(MiMoModel.forward never passes one)")


def window_of(mask, S):
    """The window a (ctx, ctx) bool mask (True = hidden) describes on its first S rows: the band i - W < j <= i, W = S for the causal mask.  Used
    only where GroupedQueryAttentionWithSink is called on its own (inside the model the window is a number and the mask is never read); one host
    read per mask object, content version and S, remembered on the tensor itself (an address would outlive the tensor).  A mask that is no such band
    is refused."""
    cache = getattr(mask, "_mimo_windows", None)
    if cache is None or cache[0] != mask._version:
        cache = (mask._version, {})
        mask._mimo_windows = cache
    if S not in cache[1]:
        if mask.dtype != torch.bool or mask.dim() != 2 or mask.shape[0] < S or mask.shape[1] < S:
            raise ValueError(f"GroupedQueryAttentionWithSink: mask must be a bool (>= {S}, >= {S}) matrix, got {mask.dtype} {tuple(mask.shape)}")
        m = mask[:S, :S]
        W = int((~m[S - 1]).sum())
        i = torch.arange(S, device=m.device).unsqueeze(1)
        j = torch.arange(S, device=m.device).unsqueeze(0)
        if W < 1 or not torch.equal(m, (j > i) | (j <= i - W)):
            raise ValueError("GroupedQueryAttentionWithSink: mask must be the causal mask or a sliding-window band (key j visible to query i iff "
                             "i - W < j <= i); the kernels compute the band from indices")
        cache[1][S] = W
    return cache[1][S]


# ----------------------------------------------------------------------------------------------- attention half
def _dims(att):
    return att.num_heads, att.num_kv_groups, att.head_dim, att.value_head_dim


def attention_forward(att, arena, h1, rt, residual=None):
    """GroupedQueryAttentionWithSink including out_proj (+ ``residual``).  h1 [M, d_in] -> ao [M, d_in] + what the backward needs."""
    Hq, Hkv, D, DV = _dims(att)
    qkv = K.gemm(L.GEMM_NT, h1, arena.fused(att.w_queries.weight, att.w_values.weight))
    qk = KM.normrope_fwd(qkv, rt.S, Hq, Hkv, D, rt.cos, rt.sin, att.q_norm.weight, att.k_norm.weight, eps=att.q_norm.eps)
    q, k, v = qk[:, : Hq * D], qk[:, Hq * D :], qkv[:, (Hq + Hkv) * D :]
    sink = att.sink if att.is_sliding_window else None
    ctx, lse = KM.sink_attn_fwd(q, k, v, rt.B, rt.S, Hq, Hkv, D, DV, rt.W, sink=sink, scale=att.att_scaling)
    ao = K.gemm(L.GEMM_NT, ctx, att.out_proj.weight, residual=residual)
    return ao, (qkv, qk, ctx, lse)


def attention_backward(att, arena, h1, saved, dao, rt, defer=None):
    """Returns dh1 [M, d_in]; writes the gradients of the four projections, the two head norms and the sink."""
    Hq, Hkv, D, DV = _dims(att)
    qkv, qk, ctx, lse = saved
    q, k, v = qk[:, : Hq * D], qk[:, Hq * D :], qkv[:, (Hq + Hkv) * D :]
    dctx = K.dgrad(dao, att.out_proj.weight)
    _wgrad(arena, att.out_proj.weight, None, dao, ctx, defer)
    dqk, dqkv = torch.empty_like(qk), torch.empty_like(qkv)
    sink = att.sink if att.is_sliding_window else None
    _, _, _, dsink = KM.sink_attn_bwd(q, k, v, ctx, dctx, lse, rt.B, rt.S, Hq, Hkv, D, DV, rt.W, sink=sink, dq=dqk[:, : Hq * D], dk=dqk[:, Hq * D :],
                                      dv=dqkv[:, (Hq + Hkv) * D :], scale=att.att_scaling)
    if sink is not None and sink.requires_grad:
        _add_vecgrad(arena, sink, dsink)
    _, dqw, dkw = KM.normrope_bwd(qkv, dqk, rt.S, Hq, Hkv, D, rt.cos, rt.sin, att.q_norm.weight, att.k_norm.weight, dx=dqkv, eps=att.q_norm.eps)
    for p, g in ((att.q_norm.weight, dqw), (att.k_norm.weight, dkw)):
        if p.requires_grad:
            _add_vecgrad(arena, p, g)
    dh1 = K.dgrad(dqkv, arena.fused(att.w_queries.weight, att.w_values.weight))
    _wgrad(arena, att.w_queries.weight, att.w_values.weight, dqkv, h1, defer)
    return dh1


# ----------------------------------------------------------------------------------------------- block
def _norm_bwd(arena, norm, x, rstd, dy, dres=None):
    gview, gacc = _vecgrad(arena, norm.weight)
    dx, _ = K.rmsnorm_bwd(x, norm.weight, rstd, dy, dres=dres, dw_out=gview, dw_accumulate=gacc)
    return dx


def block_forward(blk, x, rt, keep):
    arena = ops_dsmoe.ensure_arena(blk)
    h1, rstd1 = K.rmsnorm_fwd(x, blk.norm1.weight, eps=blk.norm1.eps)
    x2, att_saved = attention_forward(blk.att, arena, h1, rt, residual=x)
    h2, rstd2 = K.rmsnorm_fwd(x2, blk.norm2.weight, eps=blk.norm2.eps)
    if blk.use_moe:
        x3, ff_saved = ops_dsmoe.moe_forward(blk.feed_forward, arena, h2, x2, keep)
    else:
        x3, ff_saved = ops_mla.ffn_forward(blk.feed_forward, arena, h2, residual=x2)
    return x3, ((x, h1, rstd1, att_saved, x2, h2, rstd2, ff_saved) if keep else None)


def block_backward(blk, saved, dx3, rt):
    arena = ops_dsmoe.ensure_arena(blk)
    x, h1, rstd1, att_saved, x2, h2, rstd2, ff_saved = saved
    wg = []  # the weight gradients run as grouped launches at the end (their operands stay alive until then)
    if blk.use_moe:
        dh2 = ops_dsmoe.moe_backward(blk.feed_forward, arena, ff_saved, dx3, wg)
    else:
        dh2 = ops_mla.ffn_backward(blk.feed_forward, arena, h2, ff_saved, dx3, wg)
    dx2 = _norm_bwd(arena, blk.norm2, x2, rstd2, dh2, dres=dx3)
    dh1 = attention_backward(blk.att, arena, h1, att_saved, dx2, rt, wg)
    dx = _norm_bwd(arena, blk.norm1, x, rstd1, dh1, dres=dx2)
    ops_dsmoe._flush(wg)
    hook = getattr(blk, "_grad_ready", None)
    if hook is not None:
        hook(blk)
    return dx


class MiMoBlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, blk, rt, keep, *params):
        B, S, d = x.shape
        y, saved = block_forward(blk, _flat(x), rt, keep)
        ctx.blk, ctx.rt, ctx.saved, ctx.shape = blk, rt, saved, (B, S, d)
        return y.view(B, S, d)

    @staticmethod
    def backward(ctx, dy):
        if ctx.saved is None:
            raise RuntimeError("MiMoBlockFn: backward through a forward that ran without grad mode")
        dx = block_backward(ctx.blk, ctx.saved, _flat(dy), ctx.rt)
        ctx.saved = None
        return (dx.view(ctx.shape), None, None, None) + (None,) * len(ctx.blk._param_list)


def run_block(blk, x, rt):
    _check_activation(x, "MiMo TransformerBlock")
    check_bf16(blk, "MiMo TransformerBlock")
    return MiMoBlockFn.apply(x, blk, rt, torch.is_grad_enabled(), *_param_list(blk))


# ----------------------------------------------------------------------------------------------- the modules on their own
class SinkAttentionFn(torch.autograd.Function):
    """GroupedQueryAttentionWithSink.forward called outside a block."""

    @staticmethod
    def forward(ctx, x, att, rt, keep, *params):
        arena = arena_for(att)
        x2 = _flat(x)
        ao, saved = attention_forward(att, arena, x2, rt)
        ctx.att, ctx.rt, ctx.shape, ctx.saved = att, rt, x.shape, (x2, saved) if keep else None
        return ao.view(*x.shape[:-1], ao.shape[1])

    @staticmethod
    def backward(ctx, dy):
        if ctx.saved is None:
            raise RuntimeError("GroupedQueryAttentionWithSink: backward through a forward that ran without grad mode")
        x2, saved = ctx.saved
        wg = []
        dx = attention_backward(ctx.att, arena_for(ctx.att), x2, saved, _flat(dy), ctx.rt, wg)
        _flush_wgrads(wg)
        ctx.saved = None
        return (dx.view(ctx.shape), None, None, None) + (None,) * len(ctx.att._param_list)


def run_attention(att, x, rt):
    _check_activation(x, "GroupedQueryAttentionWithSink")
    check_bf16(att, "GroupedQueryAttentionWithSink")
    return SinkAttentionFn.apply(x, att, rt, torch.is_grad_enabled(), *_param_list(att))
