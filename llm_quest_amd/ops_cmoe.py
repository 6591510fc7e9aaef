"""Autograd layer of the classic MoE path: the layer (``MoE`` / ``MoE_old``) as ONE node, and ``ExpertGeLU`` used on its own.

Same construction as ``ops_moe.py`` / ``ops_latmoe.py``.  An expert is Linear(d, H) + b1 -> erf GELU -> Linear(H, d) + b2, no gate-up pair: its two
products are segmented GEMMs over all experts (``K.gemm_segmented``; weight gradients ``K.gemm_segmented_wgrad``), the plan's ``counts`` / ``offsets``
read on the device, and between / behind them ONE pass each of ``csrc/classic_moe.hip`` over the sorted buffer adds the row's expert's bias (and applies
the GELU).  The second bias is added BEFORE the combine, so ``KM.combine_fwd`` / ``combine_bwd`` serve unchanged on the biased rows.  The GELU backward
is ``mi355_gelu_bwd`` on the whole sorted buffer, the bias gradients are per-segment column sums written straight into the arena.
``MI355_MOE_SEGMENTED=0`` (``ops_moe.SEGMENTED``, read at call time) replaces the four segmented products by per-expert GEMMs behind a host read of the
counts and defers the weight gradients to the grouped launches; the row kernels are the same calls on the same buffers, so both paths give the same bits.
The softmax router with the z-loss's logsumexp, its backward and the loss are ``csrc/classic_moe.hip`` too (launchers ``kernels_cmoe.py``); plan, row
dispatch, combine and combine backward are ``csrc/moe.hip``.

Layout: an expert's four parameters sit consecutively in the arena in the module's own order (``layers.0.weight``, ``layers.0.bias``, ``layers.2.weight``,
``layers.2.bias``) and the experts follow each other at one stride, so weights, biases and their gradients reach the kernels as stacks.  The gate has
N = num_experts outputs, any value in 1..128; when that is no multiple of 8 its products run on zero-padded scratch copies (as ``ops_dsmoe``).
"""

import torch

from . import _lib as L
from . import kernels as K
from . import kernels_cmoe as KC
from . import kernels_dsmoe as KD
from . import kernels_moe as KM
from . import ops, ops_moe
from .ops_dsmoe import _forced
from .ops_g3 import _add_vecgrad, _check_activation, _flat, _param_list, check_bf16
from .ops_latmoe import _gate_weight
from .ops_moe import _loss_grad, _loss_out

BF16, F32 = torch.bfloat16, torch.float32


# ----------------------------------------------------------------------------------------------- the experts as stacks
class ExpertStacks:
    """Weights, biases and their gradients as stacks over the arena: ``w1`` [E, H, d], ``b1`` [E, 1, H], ``w2`` [E, d, H], ``b2`` [E, 1, d]; ``g*`` the same
    views of the gradient arena; ``first`` / ``last`` = the parameter range ``arena.grad_range`` covers."""

    __slots__ = ("ptrs", "w1", "b1", "w2", "b2", "gw1", "gb1", "gw2", "gb2", "first", "last", "params")


def expert_stacks(moe, arena):
    """``moe``'s stacks, rebuilt when the arena moved.  Raises unless every expert's four parameters are consecutive in the arena and the experts follow
    each other at one stride."""
    st = getattr(moe, "_cmoe_stacks", None)
    if st is not None and st.ptrs is arena._ptrs:
        return st
    lins = [(ex.layers[0], ex.layers[2]) for ex in moe.experts]
    st = ExpertStacks()
    st.w1 = K.expert_stack([a.weight.detach() for a, _ in lins])
    st.b1 = K.expert_stack([a.bias.detach().view(1, -1) for a, _ in lins])
    st.w2 = K.expert_stack([b.weight.detach() for _, b in lins])
    st.b2 = K.expert_stack([b.bias.detach().view(1, -1) for _, b in lins])
    st.first, st.last = lins[0][0].weight, lins[-1][1].bias
    i, j = arena.index(st.first), arena.index(st.last)
    if j - i + 1 != 4 * len(lins) or arena.data.storage_offset() != 0 or arena.grad.storage_offset() != 0:
        raise RuntimeError("classic MoE: the experts' parameters are not one consecutive range of the arena")
    st.params = arena.params[i : j + 1]
    for g, v in (("gw1", st.w1), ("gb1", st.b1), ("gw2", st.w2), ("gb2", st.b2)):
        setattr(st, g, arena.grad.as_strided(v.size(), v.stride(), v.storage_offset()))
    st.ptrs = arena._ptrs
    object.__setattr__(moe, "_cmoe_stacks", st)
    return st


def _segments(n_rows):
    """The per-expert path's (offset, rows) list from the counts as a host list: every start rounded up to the plan's alignment."""
    align, segs, off = KM.row_align(), [], 0
    for n in n_rows:
        segs.append((off, n))
        off += (n + align - 1) // align * align
    return segs


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


# ----------------------------------------------------------------------------------------------- the layer
def _gate_bias(moe, Ep):
    """fp32 [Ep]: ``gate.bias`` for the GEMM's bias epilogue, zero-padded to the padded gate's width."""
    b = K.cast(moe.gate.bias.detach(), F32)
    if Ep == b.numel():
        return b
    bp = torch.zeros((Ep,), dtype=F32, device=b.device)
    bp[: b.numel()].copy_(b)
    return bp


def moe_forward(moe, arena, h, keep):
    """h bf16 [T, d] contiguous -> (moe(h) [T, d], moe_loss fp32 [1], saved or None)."""
    E, k = moe.num_experts, moe.top_k
    T = h.shape[0]
    wg8 = _gate_weight(moe)
    Ep = wg8.shape[0]
    logits = K.gemm(L.GEMM_NT, h, wg8, bias=_gate_bias(moe, Ep))  # bf16(h W^T + b): one rounding after the bias is in, as addmm
    pbuf = (torch.zeros if Ep != E else torch.empty)((T, Ep), dtype=BF16, device=h.device)  # pad columns zero: the fixed-order column sums run on the pitch
    p, idx, w, s, lse = KC.route_fwd(logits[:, :E], k, _forced(moe, T, "MoE"), p=pbuf[:, :E])
    counts, offsets, slot, row_token, load = KM.plan(idx, E, KD.colsum(pbuf)[:E], moe.load_coeff)
    loss = KC.loss(lse, moe.z_router_coeff, load)
    object.__setattr__(moe, "_routed", (idx, counts))  # this forward's selection and counts, device tensors (tests and metrics; nothing here reads them back)
    xs = KM.gather_rows(h, row_token)
    segs = None if ops_moe.SEGMENTED else _segments(counts.tolist())  # the device-to-host read the segmented path does without
    pre, act, y = experts_forward(expert_stacks(moe, arena), xs, counts, offsets, T * k, segs)
    out = KM.combine_fwd(y, slot, w)
    saved = (h, xs, pre, act, y, segs, slot, row_token, w, s, idx, p, lse, counts, offsets, wg8) if keep else None
    return out, loss, saved


def moe_backward(moe, arena, saved, dout, g_loss, wg):
    """d(h) [T, d] of ``moe_forward``.  ``g_loss``: dL/d(moe_loss), fp32 [1] on the device, or None."""
    h, xs, pre, act, y, segs, slot, row_token, w, s, idx, p, lse, counts, offsets, wg8 = saved
    E = moe.num_experts
    T = h.shape[0]
    dy, dw = KM.combine_bwd(dout, row_token, slot, w, y)
    dxs = experts_backward(expert_stacks(moe, arena), arena, xs, pre, act, dy, counts, offsets, T * moe.top_k, segs, wg)
    dh = KM.combine_fwd(dxs, slot)  # the gather's backward
    # the gate: dlogits on the padded pitch (pad columns zero), dgrad on the padded weight, the weight gradient through an fp32 scratch
    Ep = wg8.shape[0]
    dlog = (torch.zeros if Ep != E else torch.empty)((T, Ep), dtype=BF16, device=h.device)
    KC.route_bwd(dw, w, s, idx, p, counts, g_loss, moe.load_coeff, moe.z_router_coeff, lse, dlogits=dlog[:, :E])
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
        _add_vecgrad(arena, gate.bias, KD.colsum(dlog)[:E])  # fixed order: per-row-part partials, then reduce_rows
    return dh


def _check(module, x, what):
    _check_activation(x, what)
    check_bf16(module, what)


class MoEFn(torch.autograd.Function):
    """``MoE.forward`` on [..., d] bf16: returns (out, moe_loss as a 0-dim tensor of the activation dtype)."""

    @staticmethod
    def forward(ctx, x, moe, keep, *params):
        arena = ops.arena_for(moe)
        out, loss, saved = moe_forward(moe, arena, _flat(x), keep)
        ctx.moe, ctx.saved, ctx.shp = moe, saved, x.shape
        ctx.set_materialize_grads(False)
        return out.view(x.shape), _loss_out(loss, x.dtype)

    @staticmethod
    def backward(ctx, dout, g_loss):
        moe, saved = ctx.moe, ctx.saved
        if saved is None:
            raise RuntimeError("MoEFn: backward through a forward that ran without grad mode")
        h = saved[0]
        dout2 = torch.zeros_like(h) if dout is None else _flat(dout)
        wg = []
        dh = moe_backward(moe, ops.arena_for(moe), saved, dout2, _loss_grad(g_loss), wg)
        ops._flush_wgrads(wg)
        ctx.saved = None
        return (dh.view(ctx.shp), None, None) + (None,) * len(moe._param_list)


def run_moe(moe, x):
    _check(moe, x, "MoE")
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


class ExpertFn(torch.autograd.Function):
    """``ExpertGeLU.forward`` called on its own."""

    @staticmethod
    def forward(ctx, x, ex, keep, *params):
        ops.arena_for(ex)
        h = _flat(x)
        y, saved = expert_forward(ex, h)
        ctx.ex, ctx.shp, ctx.saved = ex, x.shape, ((h, saved) if keep else None)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        if ctx.saved is None:
            raise RuntimeError("ExpertGeLU: backward through a forward that ran without grad mode")
        h, saved = ctx.saved
        wg = []
        dx = expert_backward(ctx.ex, ops.arena_for(ctx.ex), h, saved, _flat(dy), wg)
        ops._flush_wgrads(wg)
        ctx.saved = None
        return (dx.view(ctx.shp), None, None) + (None,) * len(ctx.ex._param_list)


def run_expert(ex, x):
    _check(ex, x, "ExpertGeLU")
    return ExpertFn.apply(x, ex, torch.is_grad_enabled(), *_param_list(ex))
