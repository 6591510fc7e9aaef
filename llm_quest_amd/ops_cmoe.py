"""Autograd layer of the classic MoE path: the layer (``MoE`` / ``MoE_old``) as ONE node, and ``ExpertGeLU`` used on its own.

What the mixture-of-experts layers share is ``ops_moe.py``'s: the padded gate, the routed core, the stack builder and the single-output node.  This file
states what is the classic layer's own.  An expert is Linear(d, H) + b1 -> erf GELU -> Linear(H, d) + b2, no gate-up pair: its two products are segmented
GEMMs over all experts (``K.gemm_segmented``; weight gradients ``K.gemm_segmented_wgrad``), the plan's ``counts`` / ``offsets`` read on the device, and
between / behind them ONE pass each of ``csrc/classic_moe.hip`` over the sorted buffer adds the row's expert's bias (and applies the GELU).  The second bias
is added BEFORE the combine, so the routed core's combine and combine backward serve unchanged on the biased rows.  The GELU backward is ``mi355_gelu_bwd``
on the whole sorted buffer, the bias gradients are per-segment column sums written straight into the arena.  ``MI355_MOE_SEGMENTED=0``
(``ops_moe.SEGMENTED``, read at call time) replaces the four segmented products by per-expert GEMMs behind a host read of the counts and defers the weight
gradients to the grouped launches; the row kernels are the same calls on the same buffers, so both paths give the same bits.  The softmax router with the
z-loss's logsumexp, its backward and the loss are ``csrc/classic_moe.hip`` too (launchers ``kernels_cmoe.py``).

Layout: an expert's four parameters sit consecutively in the arena in the module's own order (``layers.0.weight``, ``layers.0.bias``, ``layers.2.weight``,
``layers.2.bias``) and the experts follow each other at one stride, so weights, biases and their gradients reach the kernels as stacks.
"""

import torch

from . import _lib as L
from . import kernels as K
from . import kernels_cmoe as KC
from . import kernels_dsmoe as KD
from . import ops, ops_moe
from .ops_g3 import _add_vecgrad, _flat, _param_list, check_bf16  # noqa: F401  (check_bf16: re-exported for the modules)

BF16, F32 = torch.bfloat16, torch.float32


# ----------------------------------------------------------------------------------------------- the experts as stacks
def expert_stacks(moe, arena):
    """``moe``'s stacks (``ops_moe.build_stacks``): ``w1`` [E, H, d], ``b1`` [E, 1, H], ``w2`` [E, d, H], ``b2`` [E, 1, d]; ``g*`` their gradients."""
    def describe(ex):
        a, b = ex.layers[0], ex.layers[2]
        return (a.weight, a.bias, b.weight, b.bias), (a.weight.detach(), a.bias.detach().view(1, -1), b.weight.detach(), b.bias.detach().view(1, -1))

    return ops_moe.build_stacks(moe, arena, moe.experts, "classic MoE", (("w1", "gw1"), ("b1", "gb1"), ("w2", "gw2"), ("b2", "gb2")), describe)


def _product(form, a, stack, counts, offsets, max_rows, segs, N):
    """a_seg x expert e of ``stack`` for every expert: one segmented launch, or (``segs`` given) one GEMM per expert that received tokens."""
    if segs is None:
        return K.gemm_segmented(form, a, stack, counts, offsets, max_rows)
    out = torch.empty((a.shape[0], N), dtype=BF16, device=a.device)  # rows no expert writes (padding) are never read
    for e, (off, n) in enumerate(segs):
        if n:
            if form == L.GEMM_NT:
                K.gemm(L.GEMM_NT, a[off : off + n], stack[e], out=out[off : off + n])
            else:
                K.dgrad(a[off : off + n], stack[e], out=out[off : off + n])
    return out


def experts_forward(st, xs, counts, offsets, max_rows, segs):
    """(pre [R, H], act [R, H], y [R, d]) of all experts on the sorted rows ``xs``; y has the second bias in."""
    H, d = st.w1.shape[1], st.w1.shape[2]
    pre = _product(L.GEMM_NT, xs, st.w1, counts, offsets, max_rows, segs, H)
    act = KC.bias_act_fwd(pre, st.b1, counts, offsets, gelu=True)  # in place: pre = bf16(x W1^T + b1)
    y = _product(L.GEMM_NT, act, st.w2, counts, offsets, max_rows, segs, d)
    KC.bias_act_fwd(y, st.b2, counts, offsets, gelu=False)
    return pre, act, y


def experts_backward(st, arena, xs, pre, act, dy, counts, offsets, max_rows, segs, wg):
    """d(xs) [R, d]; the experts' bias gradients go straight into the arena, the weight gradients too (segmented) or are recorded in ``wg`` (per expert).
    An expert without a token ends with an exactly zero (or, accumulating, unchanged) attached gradient."""
    H, d = st.w1.shape[1], st.w1.shape[2]
    dpre = KC.gelu_bwd(pre, _product(L.GEMM_NN, dy, st.w2, counts, offsets, max_rows, segs, H))
    dxs = _product(L.GEMM_NN, dpre, st.w1, counts, offsets, max_rows, segs, d)
    need = [p.requires_grad for p in st.params]
    if all(need):
        _, acc = arena.grad_range(st.first, st.last)  # attaches every expert's .grad, resolves mixed fresh / stale states
        KC.segment_colsum(dy, counts, offsets, st.gb2, accumulate=acc)
        KC.segment_colsum(dpre, counts, offsets, st.gb1, accumulate=acc)
        if segs is None:
            K.gemm_segmented_wgrad(dy, act, counts, offsets, st.gw2, accumulate=acc)
            K.gemm_segmented_wgrad(dpre, xs, counts, offsets, st.gw1, accumulate=acc)
        else:
            for e, (off, n) in enumerate(segs):
                g2, g1 = st.gw2[e], st.gw1[e]
                if n == 0:
                    if not acc:
                        g2.zero_()
                        g1.zero_()
                    continue
                wg.append((dy[off : off + n], act[off : off + n], g2, g2 if acc else None))
                wg.append((dpre[off : off + n], xs[off : off + n], g1, g1 if acc else None))
    elif any(need):
        raise NotImplementedError("classic MoE: the experts' parameters must all be trainable or all frozen")
    return dxs


class _Experts:
    """The classic experts as ``ops_moe.routed_forward`` / ``routed_backward`` take them."""

    def __init__(self, moe, arena):
        self.st, self.arena = expert_stacks(moe, arena), arena

    def forward(self, xs, counts, offsets, max_rows):
        segs = None if ops_moe.SEGMENTED else ops_moe._segments(counts.tolist())  # the device-to-host read the segmented path does without
        pre, act, y = experts_forward(self.st, xs, counts, offsets, max_rows, segs)
        return y, (pre, act), segs

    def backward(self, r, dy, max_rows, wg):
        return experts_backward(self.st, self.arena, r.xs, *r.expert_ctx, dy, r.counts, r.offsets, max_rows, r.segs, wg)


# ----------------------------------------------------------------------------------------------- the layer
def moe_forward(moe, arena, h, keep):
    """h bf16 [T, d] contiguous -> (moe(h) [T, d], moe_loss fp32 [1], saved or None)."""
    E, T = moe.num_experts, h.shape[0]
    logits, wg8 = ops_moe.gate_forward(moe.gate, E, h)
    pbuf = ops_moe.gate_buffer(T, E, h.device)  # pad columns zero: the fixed-order column sums run on the pitch
    p, idx, w, s, lse = KC.route_fwd(logits[:, :E], moe.top_k, ops_moe._forced(moe, T, "MoE"), p=pbuf[:, :E])
    out, load, routed = ops_moe.routed_forward(_Experts(moe, arena), h, (p, idx, w, s), E, KD.colsum(pbuf)[:E], moe.load_coeff)
    loss = KC.loss(lse, moe.z_router_coeff, load)
    object.__setattr__(moe, "_routed", (idx, routed.counts))  # this forward's selection and counts, device tensors (tests and metrics; nothing here reads them back)
    return out, loss, ((h, routed, lse, wg8) if keep else None)


def moe_backward(moe, arena, saved, dout, g_loss, wg):
    """d(h) [T, d] of ``moe_forward``.  ``g_loss``: dL/d(moe_loss), fp32 [1] on the device, or None."""
    h, r, lse, wg8 = saved
    E = moe.num_experts
    dh, dw = ops_moe.routed_backward(_Experts(moe, arena), r, dout, wg)
    dlog = ops_moe.gate_buffer(h.shape[0], E, h.device)
    KC.route_bwd(dw, r.w, r.s, r.idx, r.p, r.counts, g_loss, moe.load_coeff, moe.z_router_coeff, lse, dlogits=dlog[:, :E])
    ops_moe.gate_backward(moe.gate, E, arena, h, wg8, dlog, dh, wg)
    return dh


class MoEFn(torch.autograd.Function):
    """``MoE.forward`` on [..., d] bf16: returns (out, moe_loss as a 0-dim tensor of the activation dtype)."""

    @staticmethod
    def forward(ctx, x, moe, keep, *params):
        arena = ops.arena_for(moe)
        out, loss, saved = moe_forward(moe, arena, _flat(x), keep)
        ctx.moe, ctx.saved, ctx.shp = moe, saved, x.shape
        ctx.set_materialize_grads(False)
        return out.view(x.shape), ops_moe._loss_out(loss, x.dtype)

    @staticmethod
    def backward(ctx, dout, g_loss):
        moe, saved = ctx.moe, ctx.saved
        if saved is None:
            raise RuntimeError("MoEFn: backward through a forward that ran without grad mode")
        h = saved[0]
        dout2 = torch.zeros_like(h) if dout is None else _flat(dout)
        wg = []
        dh = moe_backward(moe, ops.arena_for(moe), saved, dout2, ops_moe._loss_grad(g_loss), wg)
        ops._flush_wgrads(wg)
        ctx.saved = None
        return (dh.view(ctx.shp), None, None) + (None,) * len(moe._param_list)


def run_moe(moe, x):
    ops_moe._check(moe, x, "MoE")
    return MoEFn.apply(x, moe, torch.is_grad_enabled(), *_param_list(moe))


# ----------------------------------------------------------------------------------------------- one expert on its own (the dense path)
def expert_forward(ex, h):
    """lin2(gelu(lin1(h))) with both biases through the GEMM's bias / GELU epilogues."""
    l1, l2 = ex.layers[0], ex.layers[2]
    pre, act = K.gemm_gelu_dual(h, l1.weight.detach(), bias=K.cast(l1.bias.detach(), F32))
    return K.gemm(L.GEMM_NT, act, l2.weight.detach(), bias=K.cast(l2.bias.detach(), F32)), (pre, act)


def expert_backward(ex, arena, h, saved, dout, wg):
    pre, act = saved
    l1, l2 = ex.layers[0], ex.layers[2]
    dpre = K.gemm_dgrad_gelu_bwd(dout, l2.weight.detach(), pre)
    ops._wgrad(arena, l2.weight, None, dout, act, wg)
    if l2.bias.requires_grad:
        _add_vecgrad(arena, l2.bias, KD.colsum(dout))
    if l1.bias.requires_grad:
        _add_vecgrad(arena, l1.bias, KD.colsum(dpre))
    dh = K.gemm(L.GEMM_NN, dpre, l1.weight.detach())
    ops._wgrad(arena, l1.weight, None, dpre, h, wg)
    return dh


def _expert_node_forward(ex, arena, h, keep):
    y, saved = expert_forward(ex, h)
    return y, ((h, saved) if keep else None)


ExpertFn = ops_moe.single_output_node(  # ``ExpertGeLU.forward`` called on its own
    "ExpertGeLU", _expert_node_forward, lambda ex, arena, saved, dy, wg: expert_backward(ex, arena, *saved, dy, wg), ops.arena_for, ops._flush_wgrads)


def run_expert(ex, x):
    ops_moe._check(ex, x, "ExpertGeLU")
    return ExpertFn.apply(x, ex, torch.is_grad_enabled(), *_param_list(ex))
