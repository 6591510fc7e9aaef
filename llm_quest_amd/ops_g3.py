"""Autograd layer of the Gemma3 path (``llama3_to_gemma3/``) over the kernels of ``kernels_g3.py`` and the existing GEMMs.

Same design as ``ops.py``: activations are token-major 2-D bf16 tensors, a transformer block is ONE autograd node with a hand-written
backward, weight gradients are written by the wgrad GEMMs straight into the block's gradient arena, and the vector gradients (norm scales
and shifts, the out-projection bias) are reduced deterministically and added into it.

Block forward (x [M, d]):
    h1 = rmsnorm(x) -> qkv = h1 Wqkv^T -> RoPE + LayerNorm on the q / k heads -> windowed or causal attention -> ao = ctx Wo^T + b
    x2 = rmsnorm(ao) + x -> h2 = rmsnorm(x2) -> gu = h2 [W1 | Wg]^T -> a = GeGLU(gu) -> f = a W2^T -> x3 = rmsnorm(f) + x2
"""

import torch

from . import _lib as L
from . import kernels as K
from . import kernels_g3 as KG
from .ops import _flush_wgrads, _vecgrad, _wgrad, arena_for

BF16, F32 = torch.bfloat16, torch.float32


class Runtime:
    """Per-forward constants shared by all blocks: batch, sequence length, fp32 RoPE tables."""

    __slots__ = ("B", "S", "cos", "sin")

    def __init__(self, B, S, cos, sin):
        self.B, self.S, self.cos, self.sin = B, S, cos, sin


def rope_tables_f32(owner, cos, sin):
    """The RoPE tables as the kernels take them, fp32 and contiguous.  ``model.to(torch.bfloat16)`` casts the ``cos`` / ``sin`` buffers along with
    the parameters; the kernels multiply by bf16-rounded cos / sin anyway, so casting them back up is lossless.  Cached on ``owner`` per storage."""
    if cos.dtype == F32 and sin.dtype == F32 and cos.is_contiguous() and sin.is_contiguous():
        return cos, sin
    key = (cos.data_ptr(), sin.data_ptr(), cos.dtype, cos._version, sin._version)
    if getattr(owner, "_rope_f32_key", None) != key:
        object.__setattr__(owner, "_rope_f32", (K.cast(cos, F32), K.cast(sin, F32)))
        object.__setattr__(owner, "_rope_f32_key", key)
    return owner._rope_f32


def make_runtime(owner, B, S, cos, sin):
    if S > cos.shape[0]:
        raise ValueError(f"sequence length {S} exceeds context_length {cos.shape[0]}")
    L.require_gpu(cos, sin)
    cos, sin = rope_tables_f32(owner, cos, sin)
    return Runtime(B, S, cos, sin)


def check_bf16(module, what):
    """The path is bf16 only: the reference builds the model with cfg["dtype"] = bfloat16 and the norm parameters (created fp32) follow by .to()."""
    for name, p in module.named_parameters():
        if p.dtype != BF16:
            raise TypeError(f"{what}: parameter '{name}' is {p.dtype}; this path runs in bf16 only -- build with cfg['dtype'] = torch.bfloat16 and "
                            f"cast the model with .to(torch.bfloat16)")


def _add_vecgrad(arena, p, g_f32):
    """A reduced fp32 vector gradient into the arena's bf16 gradient of ``p``."""
    view, acc = _vecgrad(arena, p)
    if view is not None:
        K.add_f32_to_bf16(g_f32.contiguous(), view if acc else None, view)


# ----------------------------------------------------------------------------------------------- attention half
def attention_core_forward(att, q, k, v, rt):
    """Windowed layers run the sliding-window kernels; global layers the tuned causal kernels where they exist (head dims 64 and 128), else the
    windowed kernels with W = S."""
    Hq, Hkv, D = att.num_heads, att.num_kv_groups, att.head_dim
    if att.is_windowed:
        return KG.swa_attn_fwd(q, k, v, rt.B, rt.S, Hq, Hkv, D, att.window_size, scale=att.att_scaling)
    if D in (64, 128):
        return K.attn_fwd(q, k, v, rt.B, rt.S, Hq, Hkv, D, causal=True, scale=att.att_scaling)
    return KG.swa_attn_fwd(q, k, v, rt.B, rt.S, Hq, Hkv, D, max(rt.S, 1), scale=att.att_scaling)


def attention_core_backward(att, q, k, v, ctx, dctx, lse, dq, dk, dv, rt):
    Hq, Hkv, D = att.num_heads, att.num_kv_groups, att.head_dim
    if att.is_windowed:
        KG.swa_attn_bwd(q, k, v, ctx, dctx, lse, rt.B, rt.S, Hq, Hkv, D, att.window_size, dq, dk, dv, scale=att.att_scaling)
    elif D in (64, 128):
        K.attn_bwd(q, k, v, ctx, dctx, lse, rt.B, rt.S, Hq, Hkv, D, dq, dk, dv, causal=True, scale=att.att_scaling)
    else:
        KG.swa_attn_bwd(q, k, v, ctx, dctx, lse, rt.B, rt.S, Hq, Hkv, D, max(rt.S, 1), dq, dk, dv, scale=att.att_scaling)


def _norm_params(att):
    return att.q_norm.scale, att.q_norm.shift, att.k_norm.scale, att.k_norm.shift


def attention_forward(att, arena, h1, rt):
    """GroupedQueryAttention including out_proj (with its bias).  h1 [M, d] -> ao [M, d] + what the backward needs."""
    Hq, Hkv, D = att.num_heads, att.num_kv_groups, att.head_dim
    qkv = K.gemm(L.GEMM_NT, h1, arena.fused(att.w_queries.weight, att.w_values.weight))
    qk = KG.rope_ln_fwd(qkv, rt.S, Hq, Hkv, D, rt.cos, rt.sin, *_norm_params(att), eps=att.q_norm.eps)
    q, k, v = qk[:, : Hq * D], qk[:, Hq * D :], qkv[:, (Hq + Hkv) * D :]
    ctx, lse = attention_core_forward(att, q, k, v, rt)
    ao = K.gemm(L.GEMM_NT, ctx, att.out_proj.weight, bias=K.cast(att.out_proj.bias, F32))
    return ao, (qkv, qk, ctx, lse)


def attention_backward(att, arena, h1, saved, dao, rt, defer=None):
    """Returns dh1 [M, d]; writes the gradients of the projections, the bias and the two LayerNorms."""
    Hq, Hkv, D = att.num_heads, att.num_kv_groups, att.head_dim
    qkv, qk, ctx, lse = saved
    q, k, v = qk[:, : Hq * D], qk[:, Hq * D :], qkv[:, (Hq + Hkv) * D :]
    if att.out_proj.bias.requires_grad:
        _add_vecgrad(arena, att.out_proj.bias, K.colsum(dao))
    dctx = K.dgrad(dao, att.out_proj.weight)
    _wgrad(arena, att.out_proj.weight, None, dao, ctx, defer)
    dqk, dqkv = torch.empty_like(qk), torch.empty_like(qkv)
    attention_core_backward(att, q, k, v, ctx, dctx, lse, dqk[:, : Hq * D], dqk[:, Hq * D :], dqkv[:, (Hq + Hkv) * D :], rt)
    _, *grads = KG.rope_ln_bwd(qkv, dqk, rt.S, Hq, Hkv, D, rt.cos, rt.sin, *_norm_params(att), dx=dqkv, eps=att.q_norm.eps)
    for p, g in zip(_norm_params(att), grads):
        if p.requires_grad:
            _add_vecgrad(arena, p, g)
    dh1 = K.dgrad(dqkv, arena.fused(att.w_queries.weight, att.w_values.weight))
    _wgrad(arena, att.w_queries.weight, att.w_values.weight, dqkv, h1, defer)
    return dh1


# ----------------------------------------------------------------------------------------------- FFN half
def ffn_forward(ffn, arena, h2):
    F_ = ffn.lin1.weight.shape[0]
    gu = K.gemm(L.GEMM_NT, h2, arena.fused(ffn.lin1.weight, ffn.lin_gate.weight))
    a = KG.geglu_fwd(gu, F_)
    return K.gemm(L.GEMM_NT, a, ffn.lin2.weight), (gu, a)


def ffn_backward(ffn, arena, h2, saved, df, defer=None):
    F_ = ffn.lin1.weight.shape[0]
    gu, a = saved
    da = K.dgrad(df, ffn.lin2.weight)
    _wgrad(arena, ffn.lin2.weight, None, df, a, defer)
    dgu = KG.geglu_bwd(gu, da, F_)
    dh2 = K.dgrad(dgu, arena.fused(ffn.lin1.weight, ffn.lin_gate.weight))
    _wgrad(arena, ffn.lin1.weight, ffn.lin_gate.weight, dgu, h2, defer)
    return dh2


# ----------------------------------------------------------------------------------------------- block
def _norm_bwd(arena, norm, x, dy, dres=None):
    dx, dscale = KG.rmsnorm_bwd(x, norm.scale, dy, dres=dres, eps=norm.eps)
    if norm.scale.requires_grad:
        _add_vecgrad(arena, norm.scale, dscale)
    return dx


def block_forward(blk, x, rt, keep):
    arena = arena_for(blk)
    h1 = KG.rmsnorm_fwd(x, blk.pre_att_norm.scale, eps=blk.pre_att_norm.eps)
    ao, att_saved = attention_forward(blk.att, arena, h1, rt)
    x2 = KG.rmsnorm_fwd(ao, blk.post_att_norm.scale, residual=x, eps=blk.post_att_norm.eps)
    h2 = KG.rmsnorm_fwd(x2, blk.pre_ffn_norm.scale, eps=blk.pre_ffn_norm.eps)
    f, ffn_saved = ffn_forward(blk.ffn, arena, h2)
    x3 = KG.rmsnorm_fwd(f, blk.post_ffn_norm.scale, residual=x2, eps=blk.post_ffn_norm.eps)
    return x3, ((x, h1, att_saved, ao, x2, h2, ffn_saved, f) if keep else None)


def block_backward(blk, saved, dx3, rt):
    arena = arena_for(blk)
    x, h1, att_saved, ao, x2, h2, ffn_saved, f = saved
    wg = []  # the four weight-gradient GEMMs run as one grouped launch at the end
    df = _norm_bwd(arena, blk.post_ffn_norm, f, dx3)
    dh2 = ffn_backward(blk.ffn, arena, h2, ffn_saved, df, wg)
    dx2 = _norm_bwd(arena, blk.pre_ffn_norm, x2, dh2, dres=dx3)
    dao = _norm_bwd(arena, blk.post_att_norm, ao, dx2)
    dh1 = attention_backward(blk.att, arena, h1, att_saved, dao, rt, wg)
    dx = _norm_bwd(arena, blk.pre_att_norm, x, dh1, dres=dx2)
    _flush_wgrads(wg)
    hook = getattr(blk, "_grad_ready", None)
    if hook is not None:
        hook(blk)
    return dx


def _flat(x):
    x2 = x.reshape(-1, x.shape[-1])
    return x2 if x2.is_contiguous() else x2.contiguous()


class Gemma3BlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, blk, rt, keep, *params):
        B, S, d = x.shape
        y, saved = block_forward(blk, _flat(x), rt, keep)
        ctx.blk, ctx.rt, ctx.saved, ctx.shape = blk, rt, saved, (B, S, d)
        return y.view(B, S, d)

    @staticmethod
    def backward(ctx, dy):
        if ctx.saved is None:
            raise RuntimeError("Gemma3BlockFn: backward through a forward that ran without grad mode")
        dx = block_backward(ctx.blk, ctx.saved, _flat(dy), ctx.rt)
        ctx.saved = None
        return (dx.view(ctx.shape), None, None, None) + (None,) * len(ctx.blk._param_list)


def _param_list(mod):
    if not hasattr(mod, "_param_list"):
        object.__setattr__(mod, "_param_list", list(mod.parameters()))
    return mod._param_list


def _check_activation(x, what):
    L.require_gpu(x)
    if x.dtype != BF16:
        raise TypeError(f"{what} expects bf16 activations, got {x.dtype}")


def run_block(blk, x, rt):
    _check_activation(x, "Gemma3 TransformerBlock")
    check_bf16(blk, "Gemma3 TransformerBlock")
    return Gemma3BlockFn.apply(x, blk, rt, torch.is_grad_enabled(), *_param_list(blk))


# ----------------------------------------------------------------------------------------------- the modules on their own
class AttentionFn(torch.autograd.Function):
    """GroupedQueryAttention.forward called outside a block."""

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
            raise RuntimeError("GroupedQueryAttention: backward through a forward that ran without grad mode")
        x2, saved = ctx.saved
        dx = attention_backward(ctx.att, arena_for(ctx.att), x2, saved, _flat(dy), ctx.rt)
        ctx.saved = None
        return (dx.view(ctx.shape), None, None, None) + (None,) * len(ctx.att._param_list)


class FFNFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ffn, keep, *params):
        arena = arena_for(ffn)
        x2 = _flat(x)
        y, saved = ffn_forward(ffn, arena, x2)
        ctx.ffn, ctx.shape, ctx.saved = ffn, x.shape, (x2, saved) if keep else None
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        if ctx.saved is None:
            raise RuntimeError("FFN: backward through a forward that ran without grad mode")
        x2, saved = ctx.saved
        dx = ffn_backward(ctx.ffn, arena_for(ctx.ffn), x2, saved, _flat(dy))
        ctx.saved = None
        return (dx.view(ctx.shape), None, None) + (None,) * len(ctx.ffn._param_list)


class RMSNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mod, scale):
        arena_for(mod)
        x2 = _flat(x)
        ctx.mod, ctx.x2, ctx.shape = mod, x2, x.shape
        return KG.rmsnorm_fwd(x2, mod.scale, eps=mod.eps).view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        return _norm_bwd(arena_for(ctx.mod), ctx.mod, ctx.x2, _flat(dy)).view(ctx.shape), None, None


_IDENTITY_ROPE = {}


def _identity_rope(D, device):
    """cos = 1, sin = 0: the RoPE + LayerNorm kernel as a plain LayerNorm over head_dim."""
    key = (D, str(device))
    if key not in _IDENTITY_ROPE:
        _IDENTITY_ROPE[key] = (torch.ones(1, D, dtype=F32, device=device), torch.zeros(1, D, dtype=F32, device=device))
    return _IDENTITY_ROPE[key]


class LayerNormFn(torch.autograd.Function):
    """LayerNorm.forward on [..., D], D in {32, 64, 128}: every row is a head of its own."""

    @staticmethod
    def forward(ctx, x, mod, scale, shift):
        arena_for(mod)
        x2 = _flat(x)
        D = x2.shape[1]
        cos, sin = _identity_rope(D, x.device)
        ctx.mod, ctx.x2, ctx.shape = mod, x2, x.shape
        return KG.rope_ln_fwd(x2, 1, 1, 0, D, cos, sin, mod.scale, mod.shift, mod.scale, mod.shift, eps=mod.eps).view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        mod, x2 = ctx.mod, ctx.x2
        D = x2.shape[1]
        cos, sin = _identity_rope(D, x2.device)
        dx, dscale, dshift, _, _ = KG.rope_ln_bwd(x2, _flat(dy), 1, 1, 0, D, cos, sin, mod.scale, mod.shift, mod.scale, mod.shift, eps=mod.eps)
        arena = arena_for(mod)
        for p, g in ((mod.scale, dscale), (mod.shift, dshift)):
            if p.requires_grad:
                _add_vecgrad(arena, p, g)
        return dx.view(ctx.shape), None, None, None


class SlidingWindowFn(torch.autograd.Function):
    """apply_sliding_window_attention on (b, heads, s, head_dim) tensors: the transposes to token-major and back are the price of calling it on
    its own; inside a block the heads never move."""

    @staticmethod
    def forward(ctx, q, k, v, W):
        B, H, S, D = q.shape
        Hkv = k.shape[1]
        tok = lambda t, h: t.transpose(1, 2).reshape(B * S, h * D).contiguous()
        qt, kt, vt = tok(q, H), tok(k, Hkv), tok(v, Hkv)
        o, lse = KG.swa_attn_fwd(qt, kt, vt, B, S, H, Hkv, D, W)
        ctx.saved, ctx.dims = (qt, kt, vt, o, lse), (B, H, Hkv, S, D, W)
        return o.view(B, S, H, D).transpose(1, 2)

    @staticmethod
    def backward(ctx, do):
        B, H, Hkv, S, D, W = ctx.dims
        qt, kt, vt, o, lse = ctx.saved
        dot = do.transpose(1, 2).reshape(B * S, H * D).contiguous()
        dq, dk, dv = KG.swa_attn_bwd(qt, kt, vt, o, dot, lse, B, S, H, Hkv, D, W)
        back = lambda t, h: t.view(B, S, h, D).transpose(1, 2)
        return back(dq, H), back(dk, Hkv), back(dv, Hkv), None
