"""Autograd layer of the DeepSeekMoE path: the layer (``DeepSeekMoE``) and the DeepSeek-V3 block that holds one, as ONE node each.

Same construction as ``ops_moe.py``, which owns the routed experts' part: ``ops_moe.run_experts_forward`` / ``run_experts_backward`` run the products as
segmented GEMMs (gate-up + SwiGLU, ``lin2``, the two dgrads and the two weight gradients are one launch each over all routed experts, the plan's
``counts`` / ``offsets`` read on the device), so the layer's forward and backward contain no device-to-host read and their launch count does not grow with
the number of experts; ``MI355_MOE_SEGMENTED=0`` (``ops_moe.SEGMENTED``) takes the per-expert path there (one host read of the counts, two or three
launches per expert).  Plan, row dispatch, combine (one kernel; the shared experts' output is its optional addend), combine backward and router backward
are ``csrc/moe.hip`` (launchers ``kernels_moe.py``); the bias-balanced router, the bias update, the shared experts' bias + SiLU and the fixed-order column
sums of the bias gradients are ``csrc/deepseek_moe.hip`` (launchers ``kernels_dsmoe.py``).

Two layout points:
  * a routed expert is lin2(silu(lin1(x)) * lin_gate(x)): the SiLU sits on ``lin1``.  The fused gate-up kernels compute u * silu(g) on [u | g], so
    the arena holds ``lin_gate`` BEFORE ``lin1`` (``arena_named_params``); the module's parameter names and ``state_dict`` order stay upstream's.
  * the gate has N = routed experts outputs, any value in 1..128.  When that is no multiple of 8 the gate's three products (forward, dgrad, weight
    gradient) run on a zero-padded scratch copy of ``gate.weight`` / ``gate.bias`` with ceil8(N) rows, and on logits / dlogits buffers of that
    pitch whose pad columns the router never reads and the backward leaves zero.
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
from .ops_g3 import _add_vecgrad, _flat

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
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


# ----------------------------------------------------------------------------------------------- the gate
def _gate_operands(moe):
    """(weight [Ep, d] bf16, bias fp32 [Ep]) with Ep = ceil8(routed experts): the parameters themselves, or their zero-padded scratch copies."""
    E = moe.num_routed
    Ep = (E + 7) // 8 * 8
    w, b = moe.gate.weight.detach(), K.cast(moe.gate.bias.detach(), F32)
    if Ep == E:
        return w, b
    wp = torch.zeros((Ep, w.shape[1]), dtype=BF16, device=w.device)
    bp = torch.zeros((Ep,), dtype=F32, device=w.device)
    wp[:E].copy_(w)
    bp[:E].copy_(b)
    return wp, bp


def _forced(moe, T, what="DeepSeekMoE"):
    f = getattr(moe, "_forced_topk", None)
    if f is None:
        return None
    if tuple(f.shape) != (T, moe.top_k):
        raise ValueError(f"{what}: the forced selection must be (tokens, top_k) = {(T, moe.top_k)}, got {tuple(f.shape)}")
    return f.to(dtype=I32).contiguous()


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
def moe_forward(moe, arena, h, residual, keep):
    """h bf16 [T, d] contiguous -> residual + shared(h) + routed(h) [T, d]; updates ``moe.biases`` and sets ``moe.max_vio`` on the device."""
    E, k, F_ = moe.num_routed, moe.top_k, moe.routed_experts[0].hidden_dim
    T, d = h.shape
    wg8, bg8 = _gate_operands(moe)
    logits = K.gemm(L.GEMM_NT, h, wg8, bias=bg8)  # bf16(h W^T + b): one rounding after the bias is in, as addmm
    p, idx, w, s = KD.route_fwd(logits[:, :E], moe.biases, k, _forced(moe, T))
    counts, offsets, slot, row_token, _ = KM.plan(idx, E)
    max_vio = KD.bias_update(counts, moe.biases, moe.bias_update_rate)  # after this forward's router, on its stream
    object.__setattr__(moe, "max_vio", max_vio.reshape(()))
    object.__setattr__(moe, "_routed", (idx, counts))  # this forward's selection and counts, device tensors (tests and metrics; nothing here reads them back)
    xs = KM.gather_rows(h, row_token)
    # [u | g] = [lin_gate | lin1]: a = lin_gate(x) * silu(lin1(x)); segmented or per expert as ops_moe.SEGMENTED says
    y, gus, acts, segs = ops_moe.run_experts_forward(moe, arena, moe.routed_experts, "lin_gate", "lin1", xs, counts, offsets, T * k, F_)
    sh_out, sh_saved = (None, None)
    if moe.num_shared > 0:
        sh_out, sh_saved = shared_forward(moe.shared_experts, h, keep)
    out = KM.combine_fwd(y, slot, w, residual, shared=sh_out)
    saved = (h, xs, y, gus, acts, segs, slot, row_token, w, s, idx, p, counts, offsets, wg8, sh_saved) if keep else None
    return out, saved


def moe_backward(moe, arena, saved, dout, wg):
    """d(h) [T, d] of ``moe_forward`` (the residual's share is the caller's)."""
    h, xs, y, gus, acts, segs, slot, row_token, w, s, idx, p, counts, offsets, wg8, sh_saved = saved
    E, F_ = moe.num_routed, moe.routed_experts[0].hidden_dim
    T = h.shape[0]
    dy, dw = KM.combine_bwd(dout, row_token, slot, w, y)
    dxs = ops_moe.run_experts_backward(moe, arena, moe.routed_experts, "lin_gate", "lin1", xs, gus, acts, segs, dy, counts, offsets, T * moe.top_k, F_, wg)
    dh = KM.combine_fwd(dxs, slot)  # the gather's backward
    # the gate: dlogits on the padded pitch (pad columns zero), dgrad on the padded weight, the weight gradient through an fp32 scratch
    Ep = wg8.shape[0]
    dlog = (torch.zeros if Ep != E else torch.empty)((T, Ep), dtype=BF16, device=h.device)
    KM.route_bwd(dw, w, s, idx, p, dlogits=dlog[:, :E])
    K.gemm(L.GEMM_NN, dlog, wg8, out=dh, residual=dh)
    gate = moe.gate
    if gate.weight.requires_grad:
        if Ep == E:
            ops._wgrad(arena, gate.weight, None, dlog, h, wg)
        else:
            g32 = K.gemm(L.GEMM_TN, dlog, h, out_dtype=F32)  # [Ep, d]; rows E.. are zero
            view, acc = arena.grad_target(gate.weight)
            K.add_f32_to_bf16(g32[:E].reshape(-1), view if acc else None, view)
    if gate.bias.requires_grad:
        _add_vecgrad(arena, gate.bias, KD.colsum(dlog)[:E])
    if sh_saved is not None:
        dh = shared_backward(moe.shared_experts, arena, h, sh_saved, dout, wg, dh)
    return dh


def _check(module, x, what):
    ops_mla._check_activation(x, what)
    ops_mla.check_bf16(module, what)


class DeepSeekMoEFn(torch.autograd.Function):
    """``DeepSeekMoE.forward`` on [..., d] bf16."""

    @staticmethod
    def forward(ctx, x, moe, keep, *params):
        arena = ensure_arena(moe)
        h = _flat(x)
        out, saved = moe_forward(moe, arena, h, None, keep)
        ctx.moe, ctx.saved, ctx.shp = moe, saved, x.shape
        return out.view(x.shape)

    @staticmethod
    def backward(ctx, dout):
        moe, saved = ctx.moe, ctx.saved
        if saved is None:
            raise RuntimeError("DeepSeekMoEFn: backward through a forward that ran without grad mode")
        wg = []
        dh = moe_backward(moe, ensure_arena(moe), saved, _flat(dout), wg)
        _flush(wg)
        ctx.saved = None
        return (dh.view(ctx.shp), None, None) + (None,) * len(moe._param_list)


def run_moe(moe, x):
    _check(moe, x, "DeepSeekMoE")
    return DeepSeekMoEFn.apply(x, moe, torch.is_grad_enabled(), *ops_mla._param_list(moe))


class SharedExpertsFn(torch.autograd.Function):
    """``VectorizedSharedExperts.forward`` called on its own."""

    @staticmethod
    def forward(ctx, x, sh, keep, *params):
        ensure_arena(sh)
        h = _flat(x)
        out, saved = shared_forward(sh, h, keep)
        ctx.sh, ctx.saved, ctx.shp = sh, ((h, saved) if keep else None), x.shape
        return out.view(x.shape)

    @staticmethod
    def backward(ctx, dout):
        if ctx.saved is None:
            raise RuntimeError("VectorizedSharedExperts: backward through a forward that ran without grad mode")
        h, saved = ctx.saved
        wg = []
        dh = shared_backward(ctx.sh, ensure_arena(ctx.sh), h, saved, _flat(dout), wg)
        _flush(wg)
        ctx.saved = None
        return (dh.view(ctx.shp), None, None) + (None,) * len(ctx.sh._param_list)


def run_shared(sh, x):
    _check(sh, x, "VectorizedSharedExperts")
    return SharedExpertsFn.apply(x, sh, torch.is_grad_enabled(), *ops_mla._param_list(sh))


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
    _check(blk, x, "DeepSeek MoE TransformerBlock")
    return DeepSeekMoEBlockFn.apply(x, blk, rt, torch.is_grad_enabled(), *ops_mla._param_list(blk))
