"""Autograd layer of the DeepSeekMoE path: the layer (``DeepSeekMoE``) and the DeepSeek-V3 block that holds one, as ONE node each.

What the mixture-of-experts layers share is ``ops_moe.py``'s: the padded gate, the routed core (plan, row dispatch, experts, combine and their backwards),
the routed experts on segmented GEMMs or, with ``MI355_MOE_SEGMENTED=0`` (``ops_moe.SEGMENTED``), per expert, and the single-output nodes.  This file
states what is DeepSeekMoE's own: the bias-balanced router and the bias update, the shared experts (their output is the combine's optional addend), their
bias + SiLU and the fixed-order column sums of the bias gradients (``csrc/deepseek_moe.hip``, launchers ``kernels_dsmoe.py``), and the block.

Layout: a routed expert is lin2(silu(lin1(x)) * lin_gate(x)): the SiLU sits on ``lin1``.  The fused gate-up kernels compute u * silu(g) on [u | g], so
the arena holds ``lin_gate`` BEFORE ``lin1`` (``arena_named_params``); the module's parameter names and ``state_dict`` order stay upstream's.
"""

import re

import torch

from . import _lib as L
from . import kernels as K
from . import kernels_dsmoe as KD
from . import kernels_g3 as KG
from . import kernels_moe as KM
from . import ops, ops_mla, ops_moe
from .arena import ParamArena
from .ops_g3 import _add_vecgrad, _flat, _param_list

BF16 = torch.bfloat16
_LIN1 = re.compile(r"(^|\.)routed_experts\.\d+\.lin1\.weight$")


def arena_named_params(module):
    """``module.named_parameters()`` with every routed expert's ``lin_gate`` moved in front of its ``lin1`` (the fused gate-up order)."""
    named = list(module.named_parameters())
    for i in range(len(named) - 1):
        n = named[i][0]
        if _LIN1.search(n) and named[i + 1][0] == n[: -len("lin1.weight")] + "lin_gate.weight":
            named[i], named[i + 1] = named[i + 1], named[i]
    return named


def ensure_arena(module):
    """The arena of a layer or block used on its own (inside DeepSeekV3Model the model builds the block arenas the same way)."""
    if getattr(module, "_arena", None) is None:
        ar = ParamArena(arena_named_params(module))
        for m in module.modules():
            if getattr(m, "_arena", None) is None:
                object.__setattr__(m, "_arena", ar)
    return ops.arena_for(module)


# ----------------------------------------------------------------------------------------------- shared experts
def shared_forward(sh, h, keep=True):
    """sum_n lin2_n(silu(lin1_n(h))) [T, d] (lin2's biases included) + what the backward needs."""
    if sh.lin1.bias is None or sh.lin2.bias is None:
        raise NotImplementedError("VectorizedSharedExperts: only the biased form (bias=True, what DeepSeekMoE builds) has kernels")
    n, d, F_ = sh.lin1.weight.shape
    T = h.shape[0]
    w1, w2 = sh.lin1.weight.detach(), sh.lin2.weight.detach()
    z = torch.empty((T, n * F_), dtype=BF16, device=h.device)
    for i in range(n):
        K.gemm(L.GEMM_NN, h, w1[i], out=z[:, i * F_ : (i + 1) * F_])
    act = KD.bias_silu_fwd(z, sh.lin1.bias.detach().reshape(-1))  # z is the pre-activation from here on
    b2 = KD.colsum(sh.lin2.bias.detach())  # sum_n lin2.bias[n], fp32 [d]: rides on the GEMM below
    out = K.gemm(L.GEMM_NN, act, w2.view(n * F_, d), bias=b2)  # the second product AND the sum over the shared experts: K = n * hidden
    return out, ((z, act) if keep else None)


def shared_backward(sh, arena, h, saved, dout, wg, dh=None):
    """d(h) of ``shared_forward`` added into ``dh`` (a new tensor if None); parameter gradients go to the arena (weights through ``wg``)."""
    pre, act = saved
    n, d, F_ = sh.lin1.weight.shape
    w1, w2 = sh.lin1.weight.detach(), sh.lin2.weight.detach().view(n * F_, d)
    dact = K.gemm(L.GEMM_NT, dout, w2)
    dpre = KD.bias_silu_bwd(pre, dact)
    if sh.lin2.weight.requires_grad:
        view, acc = arena.grad_target(sh.lin2.weight)
        v2 = view.view(n * F_, d)
        wg.append((act, dout, v2, v2 if acc else None))
    if sh.lin2.bias.requires_grad:
        _add_vecgrad(arena, sh.lin2.bias, KD.colsum(dout).repeat(n))
    if sh.lin1.bias.requires_grad:
        _add_vecgrad(arena, sh.lin1.bias, KD.colsum(dpre))
    if sh.lin1.weight.requires_grad:
        view, acc = arena.grad_target(sh.lin1.weight)
        for i in range(n):
            wg.append((h, dpre[:, i * F_ : (i + 1) * F_], view[i], view[i] if acc else None))
    for i in range(n):
        dh = K.gemm(L.GEMM_NT, dpre[:, i * F_ : (i + 1) * F_], w1[i], out=dh, residual=dh)
    return dh


def _flush(wg):
    if ops.GROUP_WGRADS:
        ops._flush_wgrads(wg)
    else:
        for a, b, out, res in wg:
            K.gemm(L.GEMM_TN, a, b, out=out, residual=res)
        wg.clear()


# ----------------------------------------------------------------------------------------------- the layer
def _experts(moe, arena):
    """[u | g] = [lin_gate | lin1]: a = lin_gate(x) * silu(lin1(x)); segmented or per expert as ops_moe.SEGMENTED says."""
    return ops_moe.GateUpExperts(moe, arena, moe.routed_experts, "lin_gate", "lin1", moe.routed_experts[0].hidden_dim)


def moe_forward(moe, arena, h, residual, keep):
    """h bf16 [T, d] contiguous -> residual + shared(h) + routed(h) [T, d]; updates ``moe.biases`` and sets ``moe.max_vio`` on the device."""
    E, T = moe.num_routed, h.shape[0]
    logits, wg8 = ops_moe.gate_forward(moe.gate, E, h)
    route = KD.route_fwd(logits[:, :E], moe.biases, moe.top_k, ops_moe._forced(moe, T, "DeepSeekMoE"))
    sh_out, sh_saved = shared_forward(moe.shared_experts, h, keep) if moe.num_shared > 0 else (None, None)
    out, _, routed = ops_moe.routed_forward(_experts(moe, arena), h, route, E, residual=residual, shared=sh_out)
    max_vio = KD.bias_update(routed.counts, moe.biases, moe.bias_update_rate)  # after this forward's router, on its stream
    object.__setattr__(moe, "max_vio", max_vio.reshape(()))
    object.__setattr__(moe, "_routed", (routed.idx, routed.counts))  # this forward's selection and counts, device tensors (tests and metrics; nothing here reads them back)
    return out, ((h, routed, wg8, sh_saved) if keep else None)


def moe_backward(moe, arena, saved, dout, wg):
    """d(h) [T, d] of ``moe_forward`` (the residual's share is the caller's)."""
    h, r, wg8, sh_saved = saved
    E = moe.num_routed
    dh, dw = ops_moe.routed_backward(_experts(moe, arena), r, dout, wg)
    dlog = ops_moe.gate_buffer(h.shape[0], E, h.device)
    KM.route_bwd(dw, r.w, r.s, r.idx, r.p, dlogits=dlog[:, :E])
    ops_moe.gate_backward(moe.gate, E, arena, h, wg8, dlog, dh, wg)
    if sh_saved is not None:
        dh = shared_backward(moe.shared_experts, arena, h, sh_saved, dout, wg, dh)
    return dh


def _shared_node_forward(sh, arena, h, keep):
    out, saved = shared_forward(sh, h, keep)
    return out, ((h, saved) if keep else None)


DeepSeekMoEFn = ops_moe.single_output_node(  # ``DeepSeekMoE.forward`` on [..., d] bf16
    "DeepSeekMoEFn", lambda moe, arena, h, keep: moe_forward(moe, arena, h, None, keep), moe_backward, ensure_arena, _flush)
SharedExpertsFn = ops_moe.single_output_node(  # ``VectorizedSharedExperts.forward`` called on its own
    "VectorizedSharedExperts", _shared_node_forward, lambda sh, arena, saved, dout, wg: shared_backward(sh, arena, *saved, dout, wg), ensure_arena, _flush)


def run_moe(moe, x):
    ops_moe._check(moe, x, "DeepSeekMoE")
    return DeepSeekMoEFn.apply(x, moe, torch.is_grad_enabled(), *_param_list(moe))


def run_shared(sh, x):
    ops_moe._check(sh, x, "VectorizedSharedExperts")
    return SharedExpertsFn.apply(x, sh, torch.is_grad_enabled(), *_param_list(sh))


# ----------------------------------------------------------------------------------------------- the block
def block_forward(blk, x, rt, keep):
    """The dense block's attention half (ops_mla), then norm_2 and the MoE layer with the residual add on the combine."""
    arena = ensure_arena(blk)
    h1 = KG.rmsnorm_fwd(x, blk.norm_1.scale, eps=blk.norm_1.eps)
    x2, att_saved = ops_mla.attention_forward(blk.att, arena, h1, rt, residual=x)
    h2 = KG.rmsnorm_fwd(x2, blk.norm_2.scale, eps=blk.norm_2.eps)
    x3, moe_saved = moe_forward(blk.ffn, arena, h2, x2, keep)
    return x3, ((x, h1, att_saved, x2, moe_saved) if keep else None)


def block_backward(blk, saved, dx3, rt):
    arena = ensure_arena(blk)
    x, h1, att_saved, x2, moe_saved = saved
    wg = []  # the weight gradients run as grouped launches at the end (their operands stay alive until then)
    dh2 = moe_backward(blk.ffn, arena, moe_saved, dx3, wg)
    dx2 = ops_mla._norm_bwd(arena, blk.norm_2, x2, dh2, dres=dx3)
    dh1 = ops_mla.attention_backward(blk.att, arena, h1, att_saved, dx2, rt, wg)
    dx = ops_mla._norm_bwd(arena, blk.norm_1, x, dh1, dres=dx2)
    _flush(wg)
    hook = getattr(blk, "_grad_ready", None)
    if hook is not None:
        hook(blk)
    return dx


class DeepSeekMoEBlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, blk, rt, keep, *params):
        B, S, d = x.shape
        y, saved = block_forward(blk, _flat(x), rt, keep)
        ctx.blk, ctx.rt, ctx.saved, ctx.shape = blk, rt, saved, (B, S, d)
        return y.view(B, S, d)

    @staticmethod
    def backward(ctx, dy):
        if ctx.saved is None:
            raise RuntimeError("DeepSeekMoEBlockFn: backward through a forward that ran without grad mode")
        dx = block_backward(ctx.blk, ctx.saved, _flat(dy), ctx.rt)
        ctx.saved = None
        return (dx.view(ctx.shape), None, None, None) + (None,) * len(ctx.blk._param_list)


def run_block(blk, x, rt):
    ops_moe._check(blk, x, "DeepSeek MoE TransformerBlock")
    return DeepSeekMoEBlockFn.apply(x, blk, rt, torch.is_grad_enabled(), *_param_list(blk))
