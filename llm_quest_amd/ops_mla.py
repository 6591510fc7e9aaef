"""Autograd layer of the DeepSeek-V3 dense path (``llama3_to_deepseekv3/``) over the kernels of ``kernels_mla.py``, the Gemma-form RMSNorm of
``kernels_g3.py`` and the existing GEMMs.

Same design as ``ops.py`` / ``ops_g3.py``: activations are token-major 2-D bf16 tensors, a transformer block is ONE autograd node with a
hand-written backward, weight gradients are written by the wgrad GEMMs straight into the block's gradient arena, and the vector gradients
(norm scales, the seven Linear biases of the attention) are reduced deterministically and added into it.

Block forward (x [M, d]; Hq heads, Dn = d / Hq, Dr = Dn / 2):
    h1 = rmsnorm(x)
    ql = rmsnorm(h1 Wqd^T + b)  [M, 1536]      kvl = rmsnorm(h1 Wkvd^T + b)  [M, 4 Dn]      kr_pre = h1 Wkr^T + b  [M, Dr]
    [q_nope | q_rope_pre] = ql [Wq_up | Wq_decoup]^T + b           [k_nope | v] = kvl [Wk_up | Wv_up]^T + b
    (q_rope, k_rope) = RoPE(q_rope_pre, kr_pre) -> MLA attention on column slices of the two fused outputs -> x2 = ctx Wo^T + b + x
    h2 = rmsnorm(x2) -> gu = h2 [W1 | Wg]^T -> a = SwiGLU(gu) -> x3 = a W2^T + x2
The three down projections stay separate GEMMs: the latent norms read contiguous rows (``mi355_g3_rmsnorm_*`` takes no row stride).  The two up
projections are fused; their weights are concatenations rebuilt from the reference-named parameters each forward (the biases sit between the
weights in the arena), and their gradients are written per parameter from column slices of the fused output gradient.
"""

import torch

from . import _lib as L
from . import kernels as K
from . import kernels_g3 as KG
from . import kernels_mla as KM
from .ops import FUSE_SWIGLU_BWD, FUSE_SWIGLU_FWD, _flush_wgrads, _wgrad, arena_for
from .ops_g3 import Runtime, _add_vecgrad, _check_activation, _flat, _param_list, check_bf16, make_runtime  # noqa: F401  (re-exported for the modules)

BF16, F32 = torch.bfloat16, torch.float32
HEAD_DIMS = (64, 128)


def check_head_dim(head_dim):
    if head_dim not in HEAD_DIMS:
        raise ValueError(f"MultiLatentAttention: head_dim {head_dim} not built; the MLA kernels exist for head dims {HEAD_DIMS} (rope dims 32, 64)")


def check_mask(mask, S):
    """The kernels are causal by construction; a mask that is not the causal one cannot be honoured."""
    if mask is None:
        return
    key = (mask.data_ptr(), mask._version, tuple(mask.shape), S)
    if key in _MASK_OK:
        return
    m = mask[:S, :S]
    want = torch.ones(S, S, dtype=torch.bool, device=m.device).triu_(1)
    if m.dtype != torch.bool or m.shape != want.shape or not torch.equal(m, want):
        raise ValueError("MultiLatentAttention: mask must be the causal mask (True strictly above the diagonal); the MLA kernels are causal by construction")
    _MASK_OK.add(key)


_MASK_OK = set()


def _bias(lin):
    return K.cast(lin.bias, F32)


def _bias_grad(arena, lin, dy):
    if lin.bias.requires_grad:
        _add_vecgrad(arena, lin.bias, K.colsum(dy))


def _norm_bwd(arena, norm, x, dy, dres=None):
    dx, dscale = KG.rmsnorm_bwd(x, norm.scale, dy, dres=dres, eps=norm.eps)
    if norm.scale.requires_grad:
        _add_vecgrad(arena, norm.scale, dscale)
    return dx


# ----------------------------------------------------------------------------------------------- attention half
def attention_forward(att, arena, h1, rt, residual=None):
    """MultiLatentAttention including out_proj (+ ``residual``).  h1 [M, d_in] -> ao [M, d_out] + what the backward needs."""
    Hq, Dn, Dr = att.num_heads, att.head_dim, att.decoup_head_dim
    HD = Hq * Dn
    ql_pre = K.gemm(L.GEMM_NT, h1, att.wq_down_proj.weight, bias=_bias(att.wq_down_proj))
    ql = KG.rmsnorm_fwd(ql_pre, att.q_rms_norm.scale, eps=att.q_rms_norm.eps)
    kvl_pre = K.gemm(L.GEMM_NT, h1, att.wkv_down_proj.weight, bias=_bias(att.wkv_down_proj))
    kvl = KG.rmsnorm_fwd(kvl_pre, att.kv_rms_norm.scale, eps=att.kv_rms_norm.eps)
    kr_pre = K.gemm(L.GEMM_NT, h1, att.wk_decoup.weight, bias=_bias(att.wk_decoup))
    wq = torch.cat((att.wq_up_proj.weight.detach(), att.wq_decoup.weight.detach()))
    wkv = torch.cat((att.wk_up_proj.weight.detach(), att.wv_up_proj.weight.detach()))
    qcat = K.gemm(L.GEMM_NT, ql, wq, bias=torch.cat((_bias(att.wq_up_proj), _bias(att.wq_decoup))))
    kvcat = K.gemm(L.GEMM_NT, kvl, wkv, bias=torch.cat((_bias(att.wk_up_proj), _bias(att.wv_up_proj))))
    q_rope, k_rope = KM.mla_rope_fwd(qcat[:, HD:], kr_pre, rt.S, Hq, Dr, rt.cos, rt.sin)
    ctx, lse = KM.mla_attn_fwd(qcat[:, :HD], q_rope, kvcat[:, :HD], k_rope, kvcat[:, HD:], rt.B, rt.S, Hq, Dn, Dr, scale=att.att_scaling)
    ao = K.gemm(L.GEMM_NT, ctx, att.out_proj.weight, bias=_bias(att.out_proj), residual=residual)
    return ao, (ql_pre, ql, kvl_pre, kvl, wq, wkv, qcat, kvcat, q_rope, k_rope, ctx, lse)


def attention_backward(att, arena, h1, saved, dao, rt, defer=None):
    """Returns dh1 [M, d_in]; writes the gradients of the seven projections, their biases and the two latent norms."""
    Hq, Dn, Dr = att.num_heads, att.head_dim, att.decoup_head_dim
    HD = Hq * Dn
    ql_pre, ql, kvl_pre, kvl, wq, wkv, qcat, kvcat, q_rope, k_rope, ctx, lse = saved
    _bias_grad(arena, att.out_proj, dao)
    dctx = K.dgrad(dao, att.out_proj.weight)
    _wgrad(arena, att.out_proj.weight, None, dao, ctx, defer)
    dqcat, dkvcat = torch.empty_like(qcat), torch.empty_like(kvcat)
    _, dq_rope, _, dk_heads, _ = KM.mla_attn_bwd(qcat[:, :HD], q_rope, kvcat[:, :HD], k_rope, kvcat[:, HD:], ctx, dctx, lse, rt.B, rt.S, Hq, Dn, Dr,
                                                 dq_nope=dqcat[:, :HD], dk_nope=dkvcat[:, :HD], dv=dkvcat[:, HD:], scale=att.att_scaling)
    _, dkr_pre = KM.mla_rope_bwd(dq_rope, dk_heads, rt.S, Hq, Dr, rt.cos, rt.sin, dq_rope_pre=dqcat[:, HD:])
    # up projections: one dgrad each on the fused weight, the weight gradients per parameter from column slices
    if att.wq_up_proj.bias.requires_grad or att.wq_decoup.bias.requires_grad:
        gb = K.colsum(dqcat)
        for lin, g in ((att.wq_up_proj, gb[:HD]), (att.wq_decoup, gb[HD:])):
            if lin.bias.requires_grad:
                _add_vecgrad(arena, lin.bias, g)
    if att.wk_up_proj.bias.requires_grad or att.wv_up_proj.bias.requires_grad:
        gb = K.colsum(dkvcat)
        for lin, g in ((att.wk_up_proj, gb[:HD]), (att.wv_up_proj, gb[HD:])):
            if lin.bias.requires_grad:
                _add_vecgrad(arena, lin.bias, g)
    dql = K.dgrad(dqcat, wq)
    _wgrad(arena, att.wq_up_proj.weight, None, dqcat[:, :HD], ql, defer)
    _wgrad(arena, att.wq_decoup.weight, None, dqcat[:, HD:], ql, defer)
    dkvl = K.dgrad(dkvcat, wkv)
    _wgrad(arena, att.wk_up_proj.weight, None, dkvcat[:, :HD], kvl, defer)
    _wgrad(arena, att.wv_up_proj.weight, None, dkvcat[:, HD:], kvl, defer)
    dql_pre = _norm_bwd(arena, att.q_rms_norm, ql_pre, dql)
    dkvl_pre = _norm_bwd(arena, att.kv_rms_norm, kvl_pre, dkvl)
    # down projections: three products summed into one dh1 through the GEMM's residual operand, in this order
    dh1 = K.gemm(L.GEMM_NN, dql_pre, att.wq_down_proj.weight)
    K.gemm(L.GEMM_NN, dkvl_pre, att.wkv_down_proj.weight, out=dh1, residual=dh1)
    K.gemm(L.GEMM_NN, dkr_pre, att.wk_decoup.weight, out=dh1, residual=dh1)
    for lin, dy in ((att.wq_down_proj, dql_pre), (att.wkv_down_proj, dkvl_pre), (att.wk_decoup, dkr_pre)):
        _bias_grad(arena, lin, dy)
        _wgrad(arena, lin.weight, None, dy, h1, defer)
    return dh1


# ----------------------------------------------------------------------------------------------- FFN half
def ffn_forward(ffn, arena, h2, residual=None):
    F_ = ffn.lin1.weight.shape[0]
    wgu = arena.fused(ffn.lin1.weight, ffn.lin_gate.weight)
    if FUSE_SWIGLU_FWD and F_ % 32 == 0:
        gu, a = K.gemm_gateup_swiglu(h2, wgu)
    else:
        gu = K.gemm(L.GEMM_NT, h2, wgu)
        a = K.swiglu_fwd(gu, F_)
    return K.gemm(L.GEMM_NT, a, ffn.lin2.weight, residual=residual), (gu, a)


def ffn_backward(ffn, arena, h2, saved, df, defer=None):
    F_ = ffn.lin1.weight.shape[0]
    gu, a = saved
    if FUSE_SWIGLU_BWD:
        dgu = K.gemm_dgrad_swiglu_bwd(df, ffn.lin2.weight, gu)
    else:
        dgu = K.swiglu_bwd(gu, K.dgrad(df, ffn.lin2.weight), F_)
    _wgrad(arena, ffn.lin2.weight, None, df, a, defer)
    dh2 = K.dgrad(dgu, arena.fused(ffn.lin1.weight, ffn.lin_gate.weight))
    _wgrad(arena, ffn.lin1.weight, ffn.lin_gate.weight, dgu, h2, defer)
    return dh2


# ----------------------------------------------------------------------------------------------- block
def block_forward(blk, x, rt, keep):
    arena = arena_for(blk)
    h1 = KG.rmsnorm_fwd(x, blk.norm_1.scale, eps=blk.norm_1.eps)
    x2, att_saved = attention_forward(blk.att, arena, h1, rt, residual=x)
    h2 = KG.rmsnorm_fwd(x2, blk.norm_2.scale, eps=blk.norm_2.eps)
    x3, ffn_saved = ffn_forward(blk.ffn, arena, h2, residual=x2)
    return x3, ((x, h1, att_saved, x2, h2, ffn_saved) if keep else None)


def block_backward(blk, saved, dx3, rt):
    arena = arena_for(blk)
    x, h1, att_saved, x2, h2, ffn_saved = saved
    wg = []  # the ten weight-gradient GEMMs run as grouped launches at the end
    dh2 = ffn_backward(blk.ffn, arena, h2, ffn_saved, dx3, wg)
    dx2 = _norm_bwd(arena, blk.norm_2, x2, dh2, dres=dx3)
    dh1 = attention_backward(blk.att, arena, h1, att_saved, dx2, rt, wg)
    dx = _norm_bwd(arena, blk.norm_1, x, dh1, dres=dx2)
    _flush_wgrads(wg)
    hook = getattr(blk, "_grad_ready", None)
    if hook is not None:
        hook(blk)
    return dx


class DeepSeekBlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, blk, rt, keep, *params):
        B, S, d = x.shape
        y, saved = block_forward(blk, _flat(x), rt, keep)
        ctx.blk, ctx.rt, ctx.saved, ctx.shape = blk, rt, saved, (B, S, d)
        return y.view(B, S, d)

    @staticmethod
    def backward(ctx, dy):
        if ctx.saved is None:
            raise RuntimeError("DeepSeekBlockFn: backward through a forward that ran without grad mode")
        dx = block_backward(ctx.blk, ctx.saved, _flat(dy), ctx.rt)
        ctx.saved = None
        return (dx.view(ctx.shape), None, None, None) + (None,) * len(ctx.blk._param_list)


def run_block(blk, x, rt):
    _check_activation(x, "DeepSeek TransformerBlock")
    check_bf16(blk, "DeepSeek TransformerBlock")
    return DeepSeekBlockFn.apply(x, blk, rt, torch.is_grad_enabled(), *_param_list(blk))


# ----------------------------------------------------------------------------------------------- the modules on their own
class MLAFn(torch.autograd.Function):
    """MultiLatentAttention.forward called outside a block."""

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
            raise RuntimeError("MultiLatentAttention: backward through a forward that ran without grad mode")
        x2, saved = ctx.saved
        wg = []
        dx = attention_backward(ctx.att, arena_for(ctx.att), x2, saved, _flat(dy), ctx.rt, wg)
        _flush_wgrads(wg)
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


class BiasLinearFn(torch.autograd.Function):
    """y = x W^T + b on [..., K] bf16 (MTPModule.down_proj); weight and bias gradients go to the owner's arena."""

    @staticmethod
    def forward(ctx, x, lin, weight, bias):
        arena_for(lin)
        x2 = _flat(x)
        ctx.lin, ctx.x2, ctx.shape = lin, x2, x.shape
        return K.gemm(L.GEMM_NT, x2, lin.weight, bias=_bias(lin)).view(*x.shape[:-1], lin.weight.shape[0])

    @staticmethod
    def backward(ctx, dy):
        lin, arena = ctx.lin, arena_for(ctx.lin)
        dy2 = _flat(dy)
        _bias_grad(arena, lin, dy2)
        dx = K.dgrad(dy2, lin.weight)
        _wgrad(arena, lin.weight, None, dy2, ctx.x2)
        return dx.view(ctx.shape), None, None, None


class SiLUFn(torch.autograd.Function):
    """x * sigmoid(x) through the SwiGLU kernels with the linear half set to one: a = 1 * silu(x)."""

    @staticmethod
    def forward(ctx, x):
        x2 = _flat(x)
        gu = torch.cat((torch.ones_like(x2), x2), dim=1)
        ctx.gu, ctx.shape = gu, x.shape
        return K.swiglu_fwd(gu, x2.shape[1]).view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        F_ = ctx.gu.shape[1] // 2
        return K.swiglu_bwd(ctx.gu, _flat(dy), F_)[:, F_:].reshape(ctx.shape)
