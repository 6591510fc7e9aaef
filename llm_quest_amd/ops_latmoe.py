"""Autograd layer of the Nemotron-3 LatentMoE path: the layer (``LatentMoE``) as ONE node, and ``Expert`` / ``SquaredReLU`` used on their own.

Same construction as ``ops_dsmoe.py``.  ``ops_moe.run_experts_forward`` / ``run_experts_backward`` own the routed experts' part and run it with
``activation="relu2"``: the products are segmented GEMMs at the LATENT width (gate-up, ``lin2``, the two dgrads and the two weight gradients are one
launch each over all routed experts, the plan's ``counts`` / ``offsets`` read on the device), the squared-ReLU GLU between them is one pass of
``csrc/latent_moe.hip`` over the whole sorted buffer; ``MI355_MOE_SEGMENTED=0`` (``ops_moe.SEGMENTED``) takes the per-expert path there.  The sigmoid
router and its backward are ``csrc/latent_moe.hip`` too (launchers ``kernels_latmoe.py``); plan, row dispatch, combine and combine backward are
``csrc/moe.hip``, the bias update ``csrc/deepseek_moe.hip``.  The down projection, the up projection, the gate and the shared expert are the existing
GEMMs; the shared expert's output is the up projection's ``residual=`` operand, and the three dgrads into d(h) chain through it as well, so no add costs
a pass of its own.

Two layout points:
  * an expert is lin2(lin1(x) * relu(lin_gate(x))^2): the fused pair is [u | g] = [lin1 | lin_gate], the module's own parameter order, so the arena is
    ``named_parameters()`` as it stands;
  * the gate has N = routed experts outputs, any value in 1..128.  When that is no multiple of 8 the gate's three products run on a zero-padded scratch
    copy of ``gate.weight`` with ceil8(N) rows, and on logits / dlogits buffers of that pitch whose pad columns the router never reads and the backward
    leaves zero (as ``ops_dsmoe._gate_operands``).
"""

import torch

from . import _lib as L
from . import kernels as K
from . import kernels_dsmoe as KD
from . import kernels_latmoe as KL
from . import kernels_moe as KM
from . import ops, ops_moe
from .ops_dsmoe import _forced
from .ops_g3 import _check_activation, _flat, _param_list, check_bf16

BF16, F32 = torch.bfloat16, torch.float32


def _gate_weight(moe):
    """[Ep, d] bf16 with Ep = ceil8(routed experts): ``gate.weight`` itself, or its zero-padded scratch copy."""
    E = moe.num_experts
    Ep = (E + 7) // 8 * 8
    w = moe.gate.weight.detach()
    if Ep == E:
        return w
    wp = torch.zeros((Ep, w.shape[1]), dtype=BF16, device=w.device)
    wp[:E].copy_(w)
    return wp


# ----------------------------------------------------------------------------------------------- one expert (the shared one, or an Expert on its own)
def expert_forward(ex, arena, h, residual=None):
    """lin2(lin1(h) * relu(lin_gate(h))^2) [T, input_dim] (+ residual) and what the backward needs."""
    F_ = ex.hidden_dim
    gu = K.gemm(L.GEMM_NT, h, arena.fused(ex.lin1.weight, ex.lin_gate.weight))
    a = KL.relu2_glu_fwd(gu, F_)
    return K.gemm(L.GEMM_NT, a, ex.lin2.weight.detach(), residual=residual), (gu, a)


def expert_backward(ex, arena, h, saved, dout, wg, dh=None):
    """d(h) of ``expert_forward`` added into ``dh`` (a new tensor if None); the weight gradients are recorded in ``wg``."""
    gu, a = saved
    dgu = KL.relu2_glu_bwd(gu, K.gemm(L.GEMM_NN, dout, ex.lin2.weight.detach()), ex.hidden_dim)
    ops._wgrad(arena, ex.lin2.weight, None, dout, a, wg)
    dh = K.gemm(L.GEMM_NN, dgu, arena.fused(ex.lin1.weight, ex.lin_gate.weight), out=dh, residual=dh)
    ops._wgrad(arena, ex.lin1.weight, ex.lin_gate.weight, dgu, h, wg)
    return dh


# ----------------------------------------------------------------------------------------------- the layer
def moe_forward(moe, arena, h, keep):
    """h bf16 [T, d] contiguous -> shared(h) + up_proj(routed(down_proj(h))) [T, d]; in training mode updates ``moe.biases`` on the device."""
    E, k, F_ = moe.num_experts, moe.top_k, moe.routed_experts[0].hidden_dim
    T, d = h.shape
    scaling = float(moe.routed_scaling_factor)
    wg8 = _gate_weight(moe)
    logits = K.gemm(L.GEMM_NT, h, wg8)
    p, idx, w, s = KL.route_fwd(logits[:, :E], moe.biases, k, scaling, _forced(moe, T, "LatentMoE"))
    counts, offsets, slot, row_token, _ = KM.plan(idx, E)
    if moe.training:  # after this forward's router, on its stream; no host read
        object.__setattr__(moe, "max_vio", KD.bias_update(counts, moe.biases, moe.bias_update_rate).reshape(()))
    object.__setattr__(moe, "_routed", (idx, counts))  # this forward's selection and counts, device tensors (tests and metrics; nothing here reads them back)
    x_lat = K.gemm(L.GEMM_NT, h, moe.down_proj.weight.detach())
    xs = KM.gather_rows(x_lat, row_token)
    y, gus, acts, segs = ops_moe.run_experts_forward(moe, arena, moe.routed_experts, "lin1", "lin_gate", xs, counts, offsets, T * k, F_, activation="relu2")
    rl = KM.combine_fwd(y, slot, w)  # the routed sum in the latent space [T, latent]: fp32, one rounding
    sh_out, sh_saved = expert_forward(moe.shared_expert, arena, h)
    out = K.gemm(L.GEMM_NT, rl, moe.up_proj.weight.detach(), residual=sh_out)  # the add rides on the up projection
    saved = (h, xs, y, gus, acts, segs, slot, row_token, w, s, idx, p, counts, offsets, wg8, rl, sh_saved) if keep else None
    return out, saved


def moe_backward(moe, arena, saved, dout, wg):
    """d(h) [T, d] of ``moe_forward``."""
    h, xs, y, gus, acts, segs, slot, row_token, w, s, idx, p, counts, offsets, wg8, rl, sh_saved = saved
    E, F_ = moe.num_experts, moe.routed_experts[0].hidden_dim
    T = h.shape[0]
    drl = K.gemm(L.GEMM_NN, dout, moe.up_proj.weight.detach())
    ops._wgrad(arena, moe.up_proj.weight, None, dout, rl, wg)
    dy, dw = KM.combine_bwd(drl, row_token, slot, w, y)
    dxs = ops_moe.run_experts_backward(moe, arena, moe.routed_experts, "lin1", "lin_gate", xs, gus, acts, segs, dy, counts, offsets, T * moe.top_k, F_, wg,
                                       activation="relu2")
    dx_lat = KM.combine_fwd(dxs, slot)  # the gather's backward
    dh = K.gemm(L.GEMM_NN, dx_lat, moe.down_proj.weight.detach())
    ops._wgrad(arena, moe.down_proj.weight, None, dx_lat, h, wg)
    # the gate: dlogits on the padded pitch (pad columns zero), dgrad on the padded weight, the weight gradient through an fp32 scratch
    Ep = wg8.shape[0]
    dlog = (torch.zeros if Ep != E else torch.empty)((T, Ep), dtype=BF16, device=h.device)
    KL.route_bwd(dw, s, idx, p, float(moe.routed_scaling_factor), dlogits=dlog[:, :E])
    K.gemm(L.GEMM_NN, dlog, wg8, out=dh, residual=dh)
    gate = moe.gate
    if gate.weight.requires_grad:
        if Ep == E:
            ops._wgrad(arena, gate.weight, None, dlog, h, wg)
        else:
            g32 = K.gemm(L.GEMM_TN, dlog, h, out_dtype=F32)  # [Ep, d]; rows E.. are zero
            view, acc = arena.grad_target(gate.weight)
            K.add_f32_to_bf16(g32[:E].reshape(-1), view if acc else None, view)
    return expert_backward(moe.shared_expert, arena, h, sh_saved, dout, wg, dh)


def _check(module, x, what):
    _check_activation(x, what)
    check_bf16(module, what)


class LatentMoEFn(torch.autograd.Function):
    """``LatentMoE.forward`` on [..., d] bf16."""

    @staticmethod
    def forward(ctx, x, moe, keep, *params):
        arena = ops.arena_for(moe)
        out, saved = moe_forward(moe, arena, _flat(x), keep)
        ctx.moe, ctx.saved, ctx.shp = moe, saved, x.shape
        return out.view(x.shape)

    @staticmethod
    def backward(ctx, dout):
        moe, saved = ctx.moe, ctx.saved
        if saved is None:
            raise RuntimeError("LatentMoEFn: backward through a forward that ran without grad mode")
        wg = []
        dh = moe_backward(moe, ops.arena_for(moe), saved, _flat(dout), wg)
        ops._flush_wgrads(wg)
        ctx.saved = None
        return (dh.view(ctx.shp), None, None) + (None,) * len(moe._param_list)


def run_moe(moe, x):
    _check(moe, x, "LatentMoE")
    b = moe.biases
    if not b.is_cuda or b.dtype not in (BF16, F32):
        raise TypeError(f"LatentMoE: the balancing biases must be a bf16 or fp32 buffer on the GPU, got {b.dtype} on {b.device}")
    return LatentMoEFn.apply(x, moe, torch.is_grad_enabled(), *_param_list(moe))


class ExpertFn(torch.autograd.Function):
    """``Expert.forward`` called on its own."""

    @staticmethod
    def forward(ctx, x, ex, keep, *params):
        h = _flat(x)
        y, saved = expert_forward(ex, ops.arena_for(ex), h)
        ctx.ex, ctx.shp, ctx.saved = ex, x.shape, ((h, saved) if keep else None)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        if ctx.saved is None:
            raise RuntimeError("Expert: backward through a forward that ran without grad mode")
        h, saved = ctx.saved
        wg = []
        dx = expert_backward(ctx.ex, ops.arena_for(ctx.ex), h, saved, _flat(dy), wg)
        ops._flush_wgrads(wg)
        ctx.saved = None
        return (dx.view(ctx.shp), None, None) + (None,) * len(ctx.ex._param_list)


def run_expert(ex, x):
    _check(ex, x, "Expert")
    return ExpertFn.apply(x, ex, torch.is_grad_enabled(), *_param_list(ex))


class SquaredReLUFn(torch.autograd.Function):
    """relu(x)^2 on the GLU kernels with u = 1: [1 | x] -> 1 * bf16(relu(x)^2); the backward's g half is d(x)."""

    @staticmethod
    def forward(ctx, x, keep):
        h = _flat(x)
        F_ = h.shape[1]
        gu = torch.empty((h.shape[0], 2 * F_), dtype=BF16, device=h.device)
        gu[:, :F_] = 1.0
        gu[:, F_:].copy_(h)
        ctx.saved, ctx.shp = (gu if keep else None), x.shape
        return KL.relu2_glu_fwd(gu, F_).view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        if ctx.saved is None:
            raise RuntimeError("SquaredReLU: backward through a forward that ran without grad mode")
        gu = ctx.saved
        F_ = gu.shape[1] // 2
        dgu = KL.relu2_glu_bwd(gu, _flat(dy), F_)
        ctx.saved = None
        return dgu[:, F_:].reshape(ctx.shp), None


def run_relu2(x):
    _check_activation(x, "SquaredReLU")
    if x.dim() < 1 or x.shape[-1] % 8:
        raise ValueError(f"SquaredReLU: the last dimension must be a multiple of 8 (16-byte rows), got {tuple(x.shape)}")
    return SquaredReLUFn.apply(x, torch.is_grad_enabled())
