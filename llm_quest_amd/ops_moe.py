"""Autograd layer of the Qwen3 mixture-of-experts path: the layer (``Qwen3MoE``) and the block (``MoETransformerBlock``) as ONE node each.

The experts' matrix products run as segmented GEMMs (``K.gemm_segmented`` / ``K.gemm_segmented_wgrad``, csrc/gemm_segmented.hip): gate-up (+ SwiGLU), ``lin2``,
the two dgrads and the two weight gradients are ONE launch each over all experts, on the expert-sorted buffers, with the segment table (the plan's
``counts`` / ``offsets``) read on the device.  Forward and backward contain no device-to-host read and their launch count does not depend on the
number of experts.  The experts' weights and gradients reach the kernels as stacks over the block's ``ParamArena`` (``expert_stacks``: one constant
stride per expert); the weight gradients are written -- or accumulated, by ``arena.grad_target`` over the experts' parameter range -- in place, and an
expert without a token ends with an exactly zero gradient.  Everything else -- router, token-to-expert plan, row dispatch, weighted combine, their
backwards -- is ``csrc/moe.hip`` (launchers ``kernels_moe.py``).

``MI355_MOE_SEGMENTED=0`` (``SEGMENTED``, read once) keeps the earlier per-expert path for same-box A/B runs and as the tests' comparison: the host
reads the ``E`` counts once per forward, then runs two or three launches per expert that received tokens; its weight gradients go through the
caller's grouped launches.  Per segment both paths compute the same sums (the segmented kernels are bit-identical to the per-expert calls on the
128x128 tile).

This module owns the experts' part of BOTH mixture-of-experts layers: the stacks, the segmented launches, the per-expert loops and the choice between
the two paths (``run_experts_forward`` / ``run_experts_backward``) take the expert list and the names of the fused pair's two halves, so ``ops_dsmoe.py``
(routed experts, ``lin_gate`` before ``lin1``) and the two bench tools call them and restate nothing.
"""

import os

import torch

from . import _lib as L
from . import kernels as K
from . import kernels_latmoe as KL
from . import kernels_moe as KM
from . import ops

BF16, F32 = torch.bfloat16, torch.float32
SEGMENTED = os.environ.get("MI355_MOE_SEGMENTED", "1") != "0"  # 0: one launch per expert and product, behind a host read of the counts (A/B measurements, the tests' comparison)


# ----------------------------------------------------------------------------------------------- the experts as stacks
class ExpertStacks:
    """The experts' weights and gradients as 3-D stacks [E, rows, cols] over the arena (``K.expert_stack``): ``wgu`` [E, 2F, d] the fused gate-up pair,
    ``w2`` [E, d, F], ``ggu`` / ``g2`` the same views of the gradient arena; ``first`` / ``last`` = the parameter range ``arena.grad_target`` covers."""

    __slots__ = ("ptrs", "wgu", "w2", "ggu", "g2", "first", "last", "params")


def expert_stacks(owner, arena, experts, up, gate):
    """``owner``'s stacks, rebuilt when the arena moved.  ``up`` / ``gate`` name the two halves of the fused pair in the arena's order.  Raises unless every
    expert's three parameters are consecutive in the arena and the experts follow each other at one stride."""
    st = getattr(owner, "_expert_stacks", None)
    if st is not None and st.ptrs is arena._ptrs:
        return st
    pairs = [(getattr(ex, up).weight, getattr(ex, gate).weight) for ex in experts]
    st = ExpertStacks()
    st.wgu = K.expert_stack([arena.fused(a, b) for a, b in pairs])
    st.w2 = K.expert_stack([ex.lin2.weight.detach() for ex in experts])
    st.first, st.last = pairs[0][0], experts[-1].lin2.weight
    i, j = arena.index(st.first), arena.index(st.last)
    if j - i + 1 != 3 * len(experts) or arena.data.storage_offset() != 0 or arena.grad.storage_offset() != 0:
        raise RuntimeError("segmented MoE: the experts' parameters are not one consecutive range of the arena")
    st.params = arena.params[i : j + 1]
    st.ggu = arena.grad.as_strided(st.wgu.size(), st.wgu.stride(), st.wgu.storage_offset())
    st.g2 = arena.grad.as_strided(st.w2.size(), st.w2.stride(), st.w2.storage_offset())
    st.ptrs = arena._ptrs
    object.__setattr__(owner, "_expert_stacks", st)
    return st


def _check_activation(activation):
    if activation not in ("swiglu", "relu2"):
        raise ValueError(f"moe: the experts' activation must be 'swiglu' or 'relu2', got {activation!r}")
    return activation == "relu2"


def experts_forward(st, xs, counts, offsets, max_rows, F_, activation="swiglu"):
    """(gu [R, 2F], a [R, F], y [R, d]) of all experts on the sorted rows ``xs``: two launches (three when F % 32 != 0 keeps the unfused SwiGLU kernel, which
    then runs once over the whole sorted buffer; padding rows hold no defined value and are never read through slot / row_token).  ``activation``
    "relu2" (LatentMoE: a = u * relu(g)^2) always takes that unfused route, with ``KL.relu2_glu_fwd`` as the activation kernel."""
    if _check_activation(activation):
        gu = K.gemm_segmented(L.GEMM_NT, xs, st.wgu, counts, offsets, max_rows)
        a = KL.relu2_glu_fwd(gu, F_)
    elif ops.FUSE_SWIGLU_FWD and F_ % 32 == 0:
        gu, a = K.gemm_segmented(L.GEMM_NT, xs, st.wgu, counts, offsets, max_rows, epilogue="swiglu_fwd")
    else:
        gu = K.gemm_segmented(L.GEMM_NT, xs, st.wgu, counts, offsets, max_rows)
        a = K.swiglu_fwd(gu, F_)
    y = K.gemm_segmented(L.GEMM_NT, a, st.w2, counts, offsets, max_rows)
    return gu, a, y


def experts_backward(st, arena, xs, gu, a, dy, counts, offsets, max_rows, F_, activation="swiglu"):
    """d(xs) [R, d]; the experts' weight gradients go straight into the arena: two dgrad launches (+ the unfused SwiGLU backward when switched off, or the
    squared-ReLU backward for ``activation`` "relu2") and two weight-gradient launches over all experts.  An expert without a token ends with an exactly
    zero (or, accumulating, unchanged) attached gradient."""
    if _check_activation(activation):
        dgu = KL.relu2_glu_bwd(gu, K.gemm_segmented(L.GEMM_NN, dy, st.w2, counts, offsets, max_rows), F_)
    elif ops.FUSE_SWIGLU_BWD:
        dgu = K.gemm_segmented(L.GEMM_NN, dy, st.w2, counts, offsets, max_rows, epilogue="swiglu_bwd", second=gu)
    else:
        dgu = K.swiglu_bwd(gu, K.gemm_segmented(L.GEMM_NN, dy, st.w2, counts, offsets, max_rows), F_)
    dxs = K.gemm_segmented(L.GEMM_NN, dgu, st.wgu, counts, offsets, max_rows)
    need = [p.requires_grad for p in st.params]
    if all(need):
        _, acc = arena.grad_target(st.first, st.last)  # attaches every expert's .grad, resolves mixed fresh / stale states
        K.gemm_segmented_wgrad(dy, a, counts, offsets, st.g2, accumulate=acc)
        K.gemm_segmented_wgrad(dgu, xs, counts, offsets, st.ggu, accumulate=acc)
    elif any(need):
        raise NotImplementedError("segmented MoE: the experts' weights must all be trainable or all frozen (MI355_MOE_SEGMENTED=0 runs the per-expert path)")
    return dxs


# ----------------------------------------------------------------------------------------------- the per-expert path, and the choice between the two
def _experts_forward_loop(experts, up, gate, arena, xs, n_rows, F_, activation="swiglu"):
    """The per-expert path (``SEGMENTED`` off): two or three launches per expert that received tokens.  ``n_rows``: the counts as a host list (the layer's
    device-to-host read); ``experts, up, gate`` as for ``expert_stacks``.  Returns (y, gus, acts, segs)."""
    align = KM.row_align()
    y = torch.empty_like(xs)  # rows no expert writes (padding) are never read: the combine kernels go through slot / row_token
    relu2 = _check_activation(activation)
    fused = ops.FUSE_SWIGLU_FWD and F_ % 32 == 0 and not relu2
    segs, gus, acts, off = [], [], [], 0
    for ex, n in zip(experts, n_rows):
        segs.append((off, n))
        if n == 0:
            gus.append(None)
            acts.append(None)
            continue
        wgu = arena.fused(getattr(ex, up).weight, getattr(ex, gate).weight)
        if fused:  # the activation is the projection's epilogue (gu is still written: the backward needs it)
            gu, a = K.gemm_gateup_swiglu(xs[off : off + n], wgu)
        else:
            gu = K.gemm(L.GEMM_NT, xs[off : off + n], wgu)
            a = KL.relu2_glu_fwd(gu, F_) if relu2 else K.swiglu_fwd(gu, F_)
        K.gemm(L.GEMM_NT, a, ex.lin2.weight, out=y[off : off + n])
        gus.append(gu)
        acts.append(a)
        off += (n + align - 1) // align * align
    return y, gus, acts, segs


def _experts_backward_loop(experts, up, gate, arena, xs, gus, acts, segs, dy, F_, wg, activation="swiglu"):
    """The per-expert path's d(xs): the forward's segment lengths again, the weight gradients recorded in ``wg`` for the caller's grouped launches."""
    relu2 = _check_activation(activation)
    dxs = torch.empty_like(xs)  # as y: only the rows in use are read back
    for ex, (off, n), gu, a in zip(experts, segs, gus, acts):
        first, last = getattr(ex, up).weight, getattr(ex, gate).weight
        if n == 0:  # no token: a defined, exactly zero gradient (upstream leaves None; the optimizer and the gradient sync need the buffer)
            for lo, hi in ((first, last), (ex.lin2.weight, None)):
                if lo.requires_grad:
                    view, acc = arena.grad_target(lo, hi)
                    if not acc:
                        view.zero_()
            continue
        dy_e = dy[off : off + n]
        if relu2:
            dgu = KL.relu2_glu_bwd(gu, K.dgrad(dy_e, ex.lin2.weight), F_)
        elif ops.FUSE_SWIGLU_BWD:  # the activation's backward is the dgrad GEMM's epilogue
            dgu = K.gemm_dgrad_swiglu_bwd(dy_e, ex.lin2.weight, gu)
        else:
            dgu = K.swiglu_bwd(gu, K.dgrad(dy_e, ex.lin2.weight), F_)
        ops._wgrad(arena, ex.lin2.weight, None, dy_e, a, wg)
        K.dgrad(dgu, arena.fused(first, last), out=dxs[off : off + n])
        ops._wgrad(arena, first, last, dgu, xs[off : off + n], wg)
    return dxs


def run_experts_forward(owner, arena, experts, up, gate, xs, counts, offsets, max_rows, F_, activation="swiglu"):
    """All experts on the sorted rows ``xs``, on the path ``SEGMENTED`` (read here, at call time) selects.  Returns (y, gus, acts, segs), what the layers
    save: ``segs`` None = segmented (gus / acts are the whole sorted buffers), else the per-expert path's segment list.  ``activation``: "swiglu"
    (a = u * silu(g)) or "relu2" (a = u * relu(g)^2, unfused, ``csrc/latent_moe.hip``)."""
    if SEGMENTED:  # every product once over all experts, the segment table read on the device: no host read, no per-expert launch
        gus, acts, y = experts_forward(expert_stacks(owner, arena, experts, up, gate), xs, counts, offsets, max_rows, F_, activation)
        return y, gus, acts, None
    return _experts_forward_loop(experts, up, gate, arena, xs, counts.tolist(), F_, activation)  # the device-to-host read the segmented path does without


def run_experts_backward(owner, arena, experts, up, gate, xs, gus, acts, segs, dy, counts, offsets, max_rows, F_, wg, activation="swiglu"):
    """d(xs) [R, d] on the path the forward took.  Segmented, the experts' weight gradients go straight into the arena; per expert they are recorded in ``wg``."""
    if segs is None:
        return experts_backward(expert_stacks(owner, arena, experts, up, gate), arena, xs, gus, acts, dy, counts, offsets, max_rows, F_, activation)
    return _experts_backward_loop(experts, up, gate, arena, xs, gus, acts, segs, dy, F_, wg, activation)


# ----------------------------------------------------------------------------------------------- the layer
def _gate_input(moe, h, gate_probas):
    """The router's input: the gate's logits [T, E] (a column slice of a buffer whose pitch is a multiple of 8), or the replayed probabilities
    (qwen3_moe.py:115-118: cast to the activations' dtype, a constant)."""
    T, E = h.shape[0], moe.num_experts
    if gate_probas is None:
        buf = torch.empty((T, (E + 7) // 8 * 8), dtype=BF16, device=h.device)
        return K.gemm(L.GEMM_NT, h, moe.gate.weight, out=buf[:, :E]), False
    if gate_probas.dim() != 2:
        raise ValueError("gate_probas must be 2D shaped as (batch*seq, num_experts)")
    if tuple(gate_probas.shape) != (T, E):
        raise ValueError(f"gate_probas must be (batch*seq, num_experts) = {(T, E)}, got {tuple(gate_probas.shape)}")
    gp = gate_probas.detach()
    if gp.device != h.device:
        gp = gp.to(h.device)
    L.require_gpu(gp)
    return K.cast(gp.contiguous(), BF16), True


def moe_forward(moe, arena, h, residual, gate_probas, keep):
    """h bf16 [T, d] contiguous -> (residual + moe(h) [T, d], load loss fp32 [1] or None, the probabilities routed by, saved or None)."""
    E, k, F_ = moe.num_experts, moe.top_k, moe.experts[0].hidden_dim
    T, d = h.shape
    gate_in, replay = _gate_input(moe, h, gate_probas)
    p, idx, w, s = KM.route_fwd(gate_in, k, replay)
    psum = K.colsum(p) if moe.training else None
    counts, offsets, slot, row_token, loss = KM.plan(idx, E, psum, moe.load_coeff)
    xs = KM.gather_rows(h, row_token)
    y, gus, acts, segs = run_experts_forward(moe, arena, moe.experts, "lin1", "lin_gate", xs, counts, offsets, T * k, F_)
    out = KM.combine_fwd(y, slot, w, residual)
    saved = (h, xs, y, gus, acts, segs, slot, row_token, w, s, idx, p, counts, offsets, replay) if keep else None
    return out, loss, p, saved


def moe_backward(moe, arena, saved, dout, g_loss, wg):
    """d(h) [T, d] of ``moe_forward`` (the residual's share is the caller's).  ``g_loss``: dL/d(load loss), fp32 [1] on the device, or None.
    The gate's weight gradient (and, on the per-expert path, the experts') is recorded in ``wg`` for the caller's grouped launches."""
    h, xs, y, gus, acts, segs, slot, row_token, w, s, idx, p, counts, offsets, replay = saved
    F_ = moe.experts[0].hidden_dim
    dy, dw = KM.combine_bwd(dout, row_token, slot, w, None if replay else y)
    dxs = run_experts_backward(moe, arena, moe.experts, "lin1", "lin_gate", xs, gus, acts, segs, dy, counts, offsets, h.shape[0] * moe.top_k, F_, wg)
    dh = KM.combine_fwd(dxs, slot)  # the gather's backward: dh[t] = sum_j dxs[slot[t, j]]
    if not replay:  # a replayed routing is a constant: the gate is not evaluated and gets no gradient
        dlogits = KM.route_bwd(dw, w, s, idx, p, counts, g_loss, moe.load_coeff)
        K.gemm(L.GEMM_NN, dlogits, moe.gate.weight, out=dh, residual=dh)
        ops._wgrad(arena, moe.gate.weight, None, dlogits, h, wg)
    return dh


def _loss_grad(g):
    """The incoming gradient of the load loss (0-dim, the activations' dtype) as the fp32 device scalar the route backward reads."""
    return None if g is None else K.cast(g.reshape(1).contiguous(), F32)


def _loss_out(loss, dtype):
    return None if loss is None else K.cast(loss, dtype).reshape(())


class MoEFn(torch.autograd.Function):
    """``Qwen3MoE.forward`` on [..., d] bf16: returns (out, load loss or None, probabilities [T, E])."""

    @staticmethod
    def forward(ctx, x, moe, keep, gate_probas, *params):
        arena = ops.arena_for(moe)
        shp = x.shape
        h = x.reshape(-1, shp[-1])
        h = h if h.is_contiguous() else h.contiguous()
        out, loss, p, saved = moe_forward(moe, arena, h, None, gate_probas, keep)
        ctx.moe, ctx.saved, ctx.shp = moe, saved, shp
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(p)
        return out.view(shp), _loss_out(loss, x.dtype), p

    @staticmethod
    def backward(ctx, dout, g_loss, _g_p):
        moe, saved = ctx.moe, ctx.saved
        if saved is None:
            raise RuntimeError("MoEFn: backward through a forward that ran without grad mode")
        h = saved[0]
        dout2 = torch.zeros_like(h) if dout is None else dout.reshape(h.shape)
        dout2 = dout2 if dout2.is_contiguous() else dout2.contiguous()
        wg = []
        dh = moe_backward(moe, ops.arena_for(moe), saved, dout2, _loss_grad(g_loss), wg)
        ops._flush_wgrads(wg)
        ctx.saved = None
        return (dh.view(ctx.shp), None, None, None) + (None,) * len(moe._param_list)


def run_moe(moe, x, gate_probas=None):
    if not hasattr(moe, "_param_list"):
        object.__setattr__(moe, "_param_list", list(moe.parameters()))
    L.require_gpu(x)
    if x.dtype != BF16:
        raise TypeError(f"Qwen3MoE expects bf16 activations, got {x.dtype}")
    return MoEFn.apply(x, moe, torch.is_grad_enabled(), gate_probas, *moe._param_list)


# ----------------------------------------------------------------------------------------------- the block
def block_forward(blk, x, rt, keep, gate_probas):
    """The dense block's attention half (ops.attention_half_forward), then norm2 and the MoE layer with the residual add on the combine."""
    arena = ops.arena_for(blk)
    x2, att_saved = ops.attention_half_forward(blk, arena, x, rt)
    h2, rstd2 = K.rmsnorm_fwd(x2, blk.norm2.weight)
    x3, loss, p, moe_saved = moe_forward(blk.moe, arena, h2, x2, gate_probas, keep)
    saved = (x, att_saved, x2, rstd2, moe_saved) if keep else None
    return x3, loss, p, saved


def block_backward(blk, saved, dx3, g_loss, rt):
    arena = ops.arena_for(blk)
    x, att_saved, x2, rstd2, moe_saved = saved
    wg = []  # the weight gradients run as grouped launches at the end (their operands stay alive until then)
    # ---- MoE half
    dh2 = moe_backward(blk.moe, arena, moe_saved, dx3, g_loss, wg)
    gview, gacc = ops._vecgrad(arena, blk.norm2.weight)
    dx2, _ = K.rmsnorm_bwd(x2, blk.norm2.weight, rstd2, dh2, dres=dx3, dw_out=gview, dw_accumulate=gacc)
    dx = ops.attention_half_backward(blk, arena, x, att_saved, dx2, rt, wg)
    ops._flush_wgrads(wg)
    hook = getattr(blk, "_grad_ready", None)
    if hook is not None:
        hook(blk)
    return dx


class MoEBlockFn(torch.autograd.Function):
    """``MoETransformerBlock.forward`` as one node: returns (y, load loss or None, probabilities [T, E])."""

    @staticmethod
    def forward(ctx, x, blk, rt, keep, gate_probas, *params):
        B, S, d = x.shape
        x2 = x.reshape(B * S, d)
        x2 = x2 if x2.is_contiguous() else x2.contiguous()
        y, loss, p, saved = block_forward(blk, x2, rt, keep, gate_probas)
        ctx.blk, ctx.rt, ctx.saved, ctx.shape = blk, rt, saved, (B, S, d)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(p)
        return y.view(B, S, d), _loss_out(loss, x.dtype), p

    @staticmethod
    def backward(ctx, dy, g_loss, _g_p):
        B, S, d = ctx.shape
        saved = ctx.saved
        if saved is None:
            raise RuntimeError("MoEBlockFn: backward through a forward that ran without grad mode")
        dy2 = torch.zeros_like(saved[0]) if dy is None else dy.reshape(-1, d)
        dy2 = dy2 if dy2.is_contiguous() else dy2.contiguous()
        dx = block_backward(ctx.blk, saved, dy2, _loss_grad(g_loss), ctx.rt)
        ctx.saved = None
        return (dx.view(B, S, d), None, None, None, None) + (None,) * len(ctx.blk._param_list)


def run_block(blk, x, rt, gate_probas=None):
    if not hasattr(blk, "_param_list"):
        object.__setattr__(blk, "_param_list", list(blk.parameters()))
    L.require_gpu(x)
    if x.dtype != BF16:
        raise TypeError(f"Qwen3 MoE block expects bf16 activations, got {x.dtype}")
    return MoEBlockFn.apply(x, blk, rt, torch.is_grad_enabled(), gate_probas, *blk._param_list)
