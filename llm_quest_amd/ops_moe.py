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

This module also owns what the four mixture-of-experts layers (this one, ``ops_dsmoe.py``, ``ops_latmoe.py``, ``ops_cmoe.py``) have in common, stated once:
  * the experts' part of the gate-up layers: the stacks, the segmented launches, the per-expert loops and the choice between the two paths
    (``run_experts_forward`` / ``run_experts_backward``, which take the expert list and the names of the fused pair's two halves), and ``GateUpExperts``,
    the adapter the routed core drives them through; ``build_stacks`` and ``_segments`` serve the classic layer's own experts as well;
  * the routed core: ``routed_forward`` (plan, row dispatch, experts, weighted combine) and ``routed_backward`` (combine backward, experts backward, the
    gather's backward) around a ``Routed`` record of what the backward needs;
  * the padded gate: a gate has N = routed experts outputs, any value in 1..128.  When that is no multiple of 8 its three products (forward, dgrad, weight
    gradient) run on zero-padded scratch copies of ``gate.weight`` / ``gate.bias`` with ceil8(N) rows and on logits / dlogits buffers of that pitch, whose
    pad columns the routers never read and the backward leaves zero (``gate_operands``, ``gate_forward``, ``gate_buffer``, ``gate_backward``);
  * ``single_output_node``, the autograd node of a module with one output, and the small helpers ``_forced``, ``_loss_grad``, ``_loss_out``, ``_check``.
"""

import collections
import os

import torch

from . import _lib as L
from . import kernels as K
from . import kernels_dsmoe as KD
from . import kernels_latmoe as KL
from . import kernels_moe as KM
from . import ops
from .ops_g3 import _add_vecgrad, _check_activation, _flat, check_bf16

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
SEGMENTED = os.environ.get("MI355_MOE_SEGMENTED", "1") != "0"  # 0: one launch per expert and product, behind a host read of the counts (A/B measurements, the tests' comparison)


# ----------------------------------------------------------------------------------------------- the experts as stacks
class ExpertStacks:
    """The experts' parameters and gradients as 3-D stacks [E, rows, cols] over the arena (``K.expert_stack``), one attribute per name ``build_stacks`` is
    given; ``first`` / ``last`` = the parameter range ``arena.grad_target`` covers, ``params`` that range, ``ptrs`` the arena state the views belong to."""


def build_stacks(owner, arena, experts, what, names, describe):
    """``owner``'s stacks, cached on it and rebuilt when the arena moved.  ``describe(ex)`` -> (the expert's parameters in the arena's order, one tensor per
    stack); ``names``: (stack, gradient stack) per tensor, the gradient stack being the same view of the gradient arena.  Raises unless every expert's
    parameters are consecutive in the arena and the experts follow each other at one stride."""
    st = getattr(owner, "_expert_stacks", None)
    if st is not None and st.ptrs is arena._ptrs:
        return st
    params, tensors = zip(*(describe(ex) for ex in experts))
    st = ExpertStacks()
    for (name, _), per_expert in zip(names, zip(*tensors)):
        setattr(st, name, K.expert_stack(list(per_expert)))
    st.first, st.last = params[0][0], params[-1][-1]
    i, j = arena.index(st.first), arena.index(st.last)
    if j - i + 1 != len(params[0]) * len(experts) or arena.data.storage_offset() != 0 or arena.grad.storage_offset() != 0:
        raise RuntimeError(f"{what}: the experts' parameters are not one consecutive range of the arena")
    st.params = arena.params[i : j + 1]
    for name, grad in names:
        v = getattr(st, name)
        setattr(st, grad, arena.grad.as_strided(v.size(), v.stride(), v.storage_offset()))
    st.ptrs = arena._ptrs
    object.__setattr__(owner, "_expert_stacks", st)
    return st


def expert_stacks(owner, arena, experts, up, gate):
    """The gate-up experts' stacks: ``wgu`` [E, 2F, d] the fused pair, ``w2`` [E, d, F], ``ggu`` / ``g2`` their gradients.  ``up`` / ``gate`` name the two
    halves of the fused pair in the arena's order."""
    def describe(ex):
        u, g, w2 = getattr(ex, up).weight, getattr(ex, gate).weight, ex.lin2.weight
        return (u, g, w2), (arena.fused(u, g), w2.detach())

    return build_stacks(owner, arena, experts, "segmented MoE", (("wgu", "ggu"), ("w2", "g2")), describe)


def _segments(n_rows):
    """The per-expert path's (offset, rows) list from the counts as a host list: every start rounded up to the plan's alignment."""
    align, segs, off = KM.row_align(), [], 0
    for n in n_rows:
        segs.append((off, n))
        off += (n + align - 1) // align * align
    return segs


def _is_relu2(activation):
    if activation not in ("swiglu", "relu2"):
        raise ValueError(f"moe: the experts' activation must be 'swiglu' or 'relu2', got {activation!r}")
    return activation == "relu2"


def experts_forward(st, xs, counts, offsets, max_rows, F_, activation="swiglu"):
    """(gu [R, 2F], a [R, F], y [R, d]) of all experts on the sorted rows ``xs``: two launches (three when F % 32 != 0 keeps the unfused SwiGLU kernel, which
    then runs once over the whole sorted buffer; padding rows hold no defined value and are never read through slot / row_token).  ``activation``
    "relu2" (LatentMoE: a = u * relu(g)^2) always takes that unfused route, with ``KL.relu2_glu_fwd`` as the activation kernel."""
    if _is_relu2(activation):
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
    if _is_relu2(activation):
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
    y = torch.empty_like(xs)  # rows no expert writes (padding) are never read: the combine kernels go through slot / row_token
    relu2 = _is_relu2(activation)
    fused = ops.FUSE_SWIGLU_FWD and F_ % 32 == 0 and not relu2
    segs, gus, acts = _segments(n_rows), [], []
    for ex, (off, n) in zip(experts, segs):
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
    return y, gus, acts, segs


def _experts_backward_loop(experts, up, gate, arena, xs, gus, acts, segs, dy, F_, wg, activation="swiglu"):
    """The per-expert path's d(xs): the forward's segment lengths again, the weight gradients recorded in ``wg`` for the caller's grouped launches."""
    relu2 = _is_relu2(activation)
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


class GateUpExperts:
    """The routed experts of a gate-up layer as the routed core takes them: ``run_experts_forward`` / ``run_experts_backward`` (this module's, looked up
    at call time) on ``experts`` with the fused pair [``up`` | ``gate``].  The default activation is not restated in the calls."""

    def __init__(self, owner, arena, experts, up, gate, F_, activation="swiglu"):
        self.args, self.F_ = (owner, arena, experts, up, gate), F_
        self.kw = {} if activation == "swiglu" else {"activation": activation}

    def forward(self, xs, counts, offsets, max_rows):
        y, gus, acts, segs = run_experts_forward(*self.args, xs, counts, offsets, max_rows, self.F_, **self.kw)
        return y, (gus, acts), segs

    def backward(self, r, dy, max_rows, wg):
        return run_experts_backward(*self.args, r.xs, *r.expert_ctx, r.segs, dy, r.counts, r.offsets, max_rows, self.F_, wg, **self.kw)


# ----------------------------------------------------------------------------------------------- the routed core
# What ``routed_backward`` and a router's backward need of one ``routed_forward``: the sorted rows ``xs`` and the experts' output ``y`` on them, the experts'
# own saved tensors, ``segs`` (None = segmented, else the per-expert path's segment list), the plan and the router's (w, s, idx, p).
Routed = collections.namedtuple("Routed", "xs y expert_ctx segs slot row_token w s idx p counts offsets")


def routed_forward(experts, rows, route, E, psum=None, load_coeff=0.0, residual=None, shared=None):
    """Plan, row dispatch, experts, weighted combine: residual + (shared + sum_j w[t, j] experts(rows)[slot[t, j]]).  ``route``: the router's
    (p, idx, w, s); ``experts``: an object with forward(xs, counts, offsets, max_rows) -> (y, its saved tensors, segs) and backward(routed, dy, max_rows, wg)
    -> d(xs).  With ``psum`` the plan also returns the load loss.  Returns (out, load loss fp32 [1] or None, ``Routed``)."""
    p, idx, w, s = route
    counts, offsets, slot, row_token, loss = KM.plan(idx, E, psum, load_coeff)
    xs = KM.gather_rows(rows, row_token)
    y, expert_ctx, segs = experts.forward(xs, counts, offsets, idx.numel())
    out = KM.combine_fwd(y, slot, w, residual, shared=shared)
    return out, loss, Routed(xs, y, expert_ctx, segs, slot, row_token, w, s, idx, p, counts, offsets)


def routed_backward(experts, r, dout, wg, with_dw=True):
    """(d(rows) [T, width], dw fp32 [T, k] for the router's backward, None without ``with_dw``) of ``routed_forward``; the residual's and the shared addend's
    shares are the caller's.  The experts' weight gradients go into the arena or are recorded in ``wg``."""
    dy, dw = KM.combine_bwd(dout, r.row_token, r.slot, r.w, r.y if with_dw else None)
    dxs = experts.backward(r, dy, r.idx.numel(), wg)
    return KM.combine_fwd(dxs, r.slot), dw  # the gather's backward: d(rows)[t] = sum_j dxs[slot[t, j]]


# ----------------------------------------------------------------------------------------------- the padded gate
def _ceil8(E):
    return (E + 7) // 8 * 8


def gate_operands(gate, E):
    """(weight [Ep, d] bf16, bias fp32 [Ep] or None for a gate without one) with Ep = ceil8(E routed experts): the parameters themselves, or their
    zero-padded scratch copies."""
    w = gate.weight.detach()
    b = None if gate.bias is None else K.cast(gate.bias.detach(), F32)
    Ep = _ceil8(E)
    if Ep == E:
        return w, b
    wp = torch.zeros((Ep, w.shape[1]), dtype=BF16, device=w.device)
    wp[:E].copy_(w)
    if b is not None:
        bp = torch.zeros((Ep,), dtype=F32, device=w.device)
        bp[:E].copy_(b)
        b = bp
    return wp, b


def gate_forward(gate, E, h):
    """(logits [T, Ep] = bf16(h W^T + b), one rounding after the bias is in, as addmm; the weight they were computed with, for ``gate_backward``)."""
    w8, b8 = gate_operands(gate, E)
    return K.gemm(L.GEMM_NT, h, w8, bias=b8), w8


def gate_buffer(T, E, device):
    """bf16 [T, Ep] for a router to write its [:, :E] columns of (dlogits, probabilities): pad columns zero, so products and column sums run on the pitch."""
    Ep = _ceil8(E)
    return (torch.zeros if Ep != E else torch.empty)((T, Ep), dtype=BF16, device=device)


def gate_backward(gate, E, arena, h, w8, dlog, dh, wg):
    """The gate's backward from ``dlog`` [T, Ep] (a ``gate_buffer``): dh += dlog W on the padded weight, the weight gradient (recorded in ``wg``, or with a
    padded gate through an fp32 scratch) and, for a gate with a bias, the bias gradient as a fixed-order column sum."""
    K.gemm(L.GEMM_NN, dlog, w8, out=dh, residual=dh)
    if gate.weight.requires_grad:
        if w8.shape[0] == E:
            ops._wgrad(arena, gate.weight, None, dlog, h, wg)
        else:
            g32 = K.gemm(L.GEMM_TN, dlog, h, out_dtype=F32)  # [Ep, d]; rows E.. are zero
            view, acc = arena.grad_target(gate.weight)
            K.add_f32_to_bf16(g32[:E].reshape(-1), view if acc else None, view)
    if gate.bias is not None and gate.bias.requires_grad:
        _add_vecgrad(arena, gate.bias, KD.colsum(dlog)[:E])  # fixed order: per-row-part partials, then reduce_rows


# ----------------------------------------------------------------------------------------------- small helpers of the four layers
def _forced(moe, T, what):
    """The selection a test or a replay forces on the router (``moe._forced_topk``) as int32 [T, top_k], or None."""
    f = getattr(moe, "_forced_topk", None)
    if f is None:
        return None
    if tuple(f.shape) != (T, moe.top_k):
        raise ValueError(f"{what}: the forced selection must be (tokens, top_k) = {(T, moe.top_k)}, got {tuple(f.shape)}")
    return f.to(dtype=I32).contiguous()


def _loss_grad(g):
    """The incoming gradient of a layer's loss (0-dim, the activations' dtype) as the fp32 device scalar the route backward reads."""
    return None if g is None else K.cast(g.reshape(1).contiguous(), F32)


def _loss_out(loss, dtype):
    return None if loss is None else K.cast(loss, dtype).reshape(())


def _check(module, x, what):
    _check_activation(x, what)
    check_bf16(module, what)


def single_output_node(what, forward, backward, arena_of, flush):
    """The autograd node of a module called on [..., d] bf16 with one output: ``forward(module, arena, h, keep)`` -> (out [T, d], saved or None) and
    ``backward(module, arena, saved, dout, wg)`` -> d(h) on the flattened tokens; ``flush(wg)`` runs the recorded weight gradients."""

    def node_forward(ctx, x, module, keep, *params):
        out, saved = forward(module, arena_of(module), _flat(x), keep)
        ctx.module, ctx.saved, ctx.shp = module, saved, x.shape
        return out.view(x.shape)

    def node_backward(ctx, dout):
        if ctx.saved is None:
            raise RuntimeError(f"{what}: backward through a forward that ran without grad mode")
        wg = []
        dh = backward(ctx.module, arena_of(ctx.module), ctx.saved, _flat(dout), wg)
        flush(wg)
        ctx.saved = None
        return (dh.view(ctx.shp), None, None) + (None,) * len(ctx.module._param_list)

    name = what if what.endswith("Fn") else what + "Fn"  # autograd names the backward node after the class
    return type(name, (torch.autograd.Function,), dict(forward=staticmethod(node_forward), backward=staticmethod(node_backward), __module__=forward.__module__))


# ----------------------------------------------------------------------------------------------- the Qwen3 layer
def _gate_input(moe, h, gate_probas):
    """The router's input: the gate's logits [T, E] (a column slice of a buffer whose pitch is a multiple of 8), or the replayed probabilities
    (qwen3_moe.py:115-118: cast to the activations' dtype, a constant)."""
    T, E = h.shape[0], moe.num_experts
    if gate_probas is None:
        buf = torch.empty((T, _ceil8(E)), dtype=BF16, device=h.device)
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


def _experts(moe, arena):
    return GateUpExperts(moe, arena, moe.experts, "lin1", "lin_gate", moe.experts[0].hidden_dim)


def moe_forward(moe, arena, h, residual, gate_probas, keep):
    """h bf16 [T, d] contiguous -> (residual + moe(h) [T, d], load loss fp32 [1] or None, the probabilities routed by, saved or None)."""
    gate_in, replay = _gate_input(moe, h, gate_probas)
    route = KM.route_fwd(gate_in, moe.top_k, replay)
    psum = K.colsum(route[0]) if moe.training else None
    out, loss, routed = routed_forward(_experts(moe, arena), h, route, moe.num_experts, psum, moe.load_coeff, residual)
    return out, loss, route[0], ((h, routed, replay) if keep else None)


def moe_backward(moe, arena, saved, dout, g_loss, wg):
    """d(h) [T, d] of ``moe_forward`` (the residual's share is the caller's).  ``g_loss``: dL/d(load loss), fp32 [1] on the device, or None.
    The gate's weight gradient (and, on the per-expert path, the experts') is recorded in ``wg`` for the caller's grouped launches."""
    h, r, replay = saved
    dh, dw = routed_backward(_experts(moe, arena), r, dout, wg, with_dw=not replay)
    if not replay:  # a replayed routing is a constant: the gate is not evaluated and gets no gradient
        dlogits = KM.route_bwd(dw, r.w, r.s, r.idx, r.p, r.counts, g_loss, moe.load_coeff)
        K.gemm(L.GEMM_NN, dlogits, moe.gate.weight, out=dh, residual=dh)
        ops._wgrad(arena, moe.gate.weight, None, dlogits, h, wg)
    return dh


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
