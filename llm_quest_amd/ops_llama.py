"""Autograd layer of the Llama 3.2 path (``gpt_to_llama3/``) over the kernels of ``kernels_llama.py``, the Gemma-form RMSNorm of ``kernels_g3.py``,
the tuned causal attention and the existing GEMMs.

Same design as ``ops.py`` / ``ops_mla.py``: activations are token-major 2-D bf16 tensors, a transformer block is ONE autograd node with a
hand-written backward, weight gradients are written by the wgrad GEMMs straight into the block's gradient arena, and the vector gradients (norm
scales, the out-projection bias) are reduced deterministically and added into it.  No atomics: two runs give the same bits.

Block forward (x [M, d]):
    h1 = rmsnorm(x) -> qkv = h1 [Wq | Wk | Wv]^T -> (q, k) = RoPE(qkv) -> ctx = causal attention (key mask) -> x2 = ctx Wo^T + b + x
    h2 = rmsnorm(x2) -> gu = h2 [W1 | Wg]^T -> a = SwiGLU(gu) -> x3 = a W2^T + x2
With ``att.track_max_attn_logit`` the per-head maximum attention logit of the post-RoPE q, k is left in ``att.max_attn_logit`` (one more launch).
With ``att.expose_qk`` and grad mode on, the block's (and the attention's) autograd node returns the post-RoPE q, k as two more differentiable
outputs, left in ``att.exposed_qk`` (what ``common/reinforced_attention_learning.py`` reads); the gradients that arrive on them are added to dq, dk
ahead of the RoPE backward.  With the flag off the node has one output and launches what it launched before the flag existed.
"""

import torch

from . import _lib as L
from . import kernels as K
from . import kernels_g3 as KG
from . import kernels_llama as KL
from . import kernels_ral as KR
from .ops import _flush_wgrads, _wgrad, arena_for
from .ops import make_runtime as _make_runtime
from .ops_g3 import _add_vecgrad, _check_activation, _flat, _param_list, rope_tables_f32
from .ops_mla import FFNFn, SiLUFn, _norm_bwd, ffn_backward, ffn_forward  # noqa: F401  (the SwiGLU FFN is DeepSeek's; re-exported for the modules)

BF16, F32 = torch.bfloat16, torch.float32
HEAD_DIMS = KL.HEAD_DIMS


def check_head_dim(head_dim):
    if head_dim not in HEAD_DIMS:
        raise ValueError(f"GroupedQueryAttention: head_dim {head_dim} not built; the Llama kernels exist for head dims {HEAD_DIMS}")


def check_bf16(module, what):
    """The path is bf16 only: upstream's 1B config builds bf16 Linears and the norm scales (created fp32) follow by .to()."""
    for name, p in module.named_parameters():
        if p.dtype != BF16:
            raise TypeError(f"{what}: parameter '{name}' is {p.dtype}; this path runs in bf16 only -- cast the model with .to(torch.bfloat16)")


def make_runtime(owner, B, S, cos, sin, attn_mask=None):
    """The ``ops.Runtime`` of a forward (shape, positions, key mask, RoPE tables) on the model's buffers: the tables go back to fp32 when ``.to(bfloat16)``
    has cast them.  ``attn_mask``: (b, s), True = a real token (a key that may be attended), as the reference's ``attn_mask``."""
    L.require_gpu(cos, sin, attn_mask)
    return _make_runtime(B, S, cos.device, *rope_tables_f32(owner, cos, sin), attn_mask)


# ----------------------------------------------------------------------------------------------- attention half
def attention_forward(att, arena, h1, rt, residual=None):
    """GroupedQueryAttention including out_proj with its bias (+ ``residual``).  h1 [M, d_in] -> ao [M, d_out] + what the backward needs."""
    Hq, Hkv, D = att.num_heads, att.num_kv_groups, att.head_dim
    qkv = K.gemm(L.GEMM_NT, h1, arena.fused(att.w_queries.weight, att.w_values.weight))
    q, k = KL.rope_fwd(qkv, rt.cos, rt.sin, rt.pos, Hq, Hkv, D)
    v = qkv[:, (Hq + Hkv) * D :]
    if att.track_max_attn_logit:
        att.max_attn_logit = KL.attn_max_logit(q, k, rt.B, rt.S, Hq, Hkv, D, key_mask=rt.key_mask, scale=att.att_scaling)
    ctx, lse = K.attn_fwd(q, k, v, rt.B, rt.S, Hq, Hkv, D, key_mask=rt.key_mask, causal=True, scale=att.att_scaling)
    ao = K.gemm(L.GEMM_NT, ctx, att.out_proj.weight, bias=K.cast(att.out_proj.bias, F32), residual=residual)
    return ao, (qkv, q, k, ctx, lse)


def attention_backward(att, arena, h1, saved, dao, rt, defer=None, qk_grads=(None, None)):
    """Returns dh1 [M, d_in]; writes the gradients of the four projections and the bias.  ``qk_grads``: what arrived on the exposed q, k (None = zero)."""
    Hq, Hkv, D = att.num_heads, att.num_kv_groups, att.head_dim
    qkv, q, k, ctx, lse = saved
    v = qkv[:, (Hq + Hkv) * D :]
    if att.out_proj.bias.requires_grad:
        _add_vecgrad(arena, att.out_proj.bias, K.colsum(dao))
    dctx = K.dgrad(dao, att.out_proj.weight)
    _wgrad(arena, att.out_proj.weight, None, dao, ctx, defer)
    dqkv, dq, dk = torch.empty_like(qkv), torch.empty_like(q), torch.empty_like(k)
    K.attn_bwd(q, k, v, ctx, dctx, lse, rt.B, rt.S, Hq, Hkv, D, dq, dk, dqkv[:, (Hq + Hkv) * D :], key_mask=rt.key_mask, causal=True, scale=att.att_scaling)
    for d, extra in zip((dq, dk), qk_grads):
        if extra is not None:
            KR.add_bf16_(d, extra.reshape(d.shape).contiguous())
    KL.rope_bwd(dq, dk, rt.cos, rt.sin, rt.pos, dqkv, Hq, Hkv, D)
    dh1 = K.dgrad(dqkv, arena.fused(att.w_queries.weight, att.w_values.weight))
    _wgrad(arena, att.w_queries.weight, att.w_values.weight, dqkv, h1, defer)
    return dh1


# ----------------------------------------------------------------------------------------------- block
def block_forward(blk, x, rt, keep):
    arena = arena_for(blk)
    h1 = KG.rmsnorm_fwd(x, blk.norm_1.scale, eps=blk.norm_1.eps)
    x2, att_saved = attention_forward(blk.att, arena, h1, rt, residual=x)
    h2 = KG.rmsnorm_fwd(x2, blk.norm_2.scale, eps=blk.norm_2.eps)
    x3, ffn_saved = ffn_forward(blk.ffn, arena, h2, residual=x2)
    return x3, ((x, h1, att_saved, x2, h2, ffn_saved) if keep else None)


def block_backward(blk, saved, dx3, rt, qk_grads=(None, None)):
    arena = arena_for(blk)
    x, h1, att_saved, x2, h2, ffn_saved = saved
    wg = []  # the four weight-gradient GEMMs run as one grouped launch at the end
    dh2 = ffn_backward(blk.ffn, arena, h2, ffn_saved, dx3, wg)
    dx2 = _norm_bwd(arena, blk.norm_2, x2, dh2, dres=dx3)
    dh1 = attention_backward(blk.att, arena, h1, att_saved, dx2, rt, wg, qk_grads)
    dx = _norm_bwd(arena, blk.norm_1, x, dh1, dres=dx2)
    _flush_wgrads(wg)
    hook = getattr(blk, "_grad_ready", None)
    if hook is not None:
        hook(blk)
    return dx


def _exposes(att, keep):
    return bool(keep and getattr(att, "expose_qk", False))


def _with_exposed(ctx, y, att_saved, expose):
    """The node's outputs: y, and with ``expose`` the post-RoPE q, k of ``attention_forward``'s saved tuple (aliases: the saved tensors stay plain)."""
    ctx.exposed = expose
    if not expose:
        return y
    ctx.set_materialize_grads(False)  # a gradient that never arrived stays None and costs no launch
    return y, att_saved[1].detach(), att_saved[2].detach()


def _leave_exposed(att, out):
    """y of a node's outputs; q, k (if the node returned them) go to ``att.exposed_qk``."""
    if isinstance(out, tuple):
        att.exposed_qk = (out[1], out[2])
        return out[0]
    att.exposed_qk = None
    return out


class LlamaBlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, blk, rt, keep, *params):
        B, S, d = x.shape
        y, saved = block_forward(blk, _flat(x), rt, keep)
        ctx.blk, ctx.rt, ctx.saved, ctx.shape = blk, rt, saved, (B, S, d)
        return _with_exposed(ctx, y.view(B, S, d), saved[2] if keep else None, _exposes(blk.att, keep))

    @staticmethod
    def backward(ctx, dy, *dqk):
        if ctx.saved is None:
            raise RuntimeError("LlamaBlockFn: backward through a forward that ran without grad mode")
        if dy is None:  # only with exposed q, k: nothing but they reached the loss
            dy = torch.zeros(ctx.shape, dtype=BF16, device=ctx.saved[0].device)
        dx = block_backward(ctx.blk, ctx.saved, _flat(dy), ctx.rt, dqk if ctx.exposed else (None, None))
        ctx.saved = None
        return (dx.view(ctx.shape), None, None, None) + (None,) * len(ctx.blk._param_list)


def run_block(blk, x, rt):
    _check_activation(x, "Llama TransformerBlock")
    check_bf16(blk, "Llama TransformerBlock")
    return _leave_exposed(blk.att, LlamaBlockFn.apply(x, blk, rt, torch.is_grad_enabled(), *_param_list(blk)))


class GQAFn(torch.autograd.Function):
    """GroupedQueryAttention.forward called outside a block."""

    @staticmethod
    def forward(ctx, x, att, rt, keep, *params):
        arena = arena_for(att)
        x2 = _flat(x)
        ao, saved = attention_forward(att, arena, x2, rt)
        ctx.att, ctx.rt, ctx.shape, ctx.saved = att, rt, x.shape, (x2, saved) if keep else None
        ctx.oshape = (*x.shape[:-1], ao.shape[1])
        return _with_exposed(ctx, ao.view(ctx.oshape), saved, _exposes(att, keep))

    @staticmethod
    def backward(ctx, dy, *dqk):
        if ctx.saved is None:
            raise RuntimeError("GroupedQueryAttention: backward through a forward that ran without grad mode")
        x2, saved = ctx.saved
        if dy is None:
            dy = torch.zeros(ctx.oshape, dtype=BF16, device=x2.device)
        wg = []
        dx = attention_backward(ctx.att, arena_for(ctx.att), x2, saved, _flat(dy), ctx.rt, wg, dqk if ctx.exposed else (None, None))
        _flush_wgrads(wg)
        ctx.saved = None
        return (dx.view(ctx.shape), None, None, None) + (None,) * len(ctx.att._param_list)


def run_attention(att, x, rt):
    return _leave_exposed(att, GQAFn.apply(x, att, rt, torch.is_grad_enabled(), *_param_list(att)))
