"""Autograd layer of the Nemotron-3 LatentMoE path: the layer (``LatentMoE``) as ONE node, and ``Expert`` / ``SquaredReLU`` used on their own.

What the mixture-of-experts layers share is ``ops_moe.py``'s: the padded gate, the routed core, the routed experts (here with ``activation="relu2"``:
segmented GEMMs at the LATENT width, the squared-ReLU GLU between them one pass of ``csrc/latent_moe.hip`` over the whole sorted buffer; per expert with
``ops_moe.SEGMENTED`` off) and the single-output nodes.  This file states what is LatentMoE's own: the sigmoid router and its backward
(``csrc/latent_moe.hip``, launchers ``kernels_latmoe.py``), the bias update (``csrc/deepseek_moe.hip``), and the down projection, the up projection and the
shared expert on the existing GEMMs; the shared expert's output is the up projection's ``residual=`` operand, and the three dgrads into d(h) chain through
it as well, so no add costs a pass of its own.

Layout: an expert is lin2(lin1(x) * relu(lin_gate(x))^2): the fused pair is [u | g] = [lin1 | lin_gate], the module's own parameter order, so the arena is
``named_parameters()`` as it stands.
"""

import torch

from . import _lib as L
from . import kernels as K
from . import kernels_dsmoe as KD
from . import kernels_latmoe as KL
from . import ops, ops_moe
from .ops_g3 import _check_activation, _flat, _param_list

BF16, F32 = torch.bfloat16, torch.float32


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
def _experts(moe, arena):
    return ops_moe.GateUpExperts(moe, arena, moe.routed_experts, "lin1", "lin_gate", moe.routed_experts[0].hidden_dim, "relu2")


def moe_forward(moe, arena, h, keep):
    """h bf16 [T, d] contiguous -> shared(h) + up_proj(routed(down_proj(h))) [T, d]; in training mode updates ``moe.biases`` on the device."""
    E, T = moe.num_experts, h.shape[0]
    logits, wg8 = ops_moe.gate_forward(moe.gate, E, h)
    route = KL.route_fwd(logits[:, :E], moe.biases, moe.top_k, float(moe.routed_scaling_factor), ops_moe._forced(moe, T, "LatentMoE"))
    x_lat = K.gemm(L.GEMM_NT, h, moe.down_proj.weight.detach())
    rl, _, routed = ops_moe.routed_forward(_experts(moe, arena), x_lat, route, E)  # the routed sum in the latent space [T, latent]: fp32, one rounding
    if moe.training:  # after this forward's router, on its stream; no host read
        object.__setattr__(moe, "max_vio", KD.bias_update(routed.counts, moe.biases, moe.bias_update_rate).reshape(()))
    object.__setattr__(moe, "_routed", (routed.idx, routed.counts))  # this forward's selection and counts, device tensors (tests and metrics; nothing here reads them back)
    sh_out, sh_saved = expert_forward(moe.shared_expert, arena, h)
    out = K.gemm(L.GEMM_NT, rl, moe.up_proj.weight.detach(), residual=sh_out)  # the add rides on the up projection
    return out, ((h, routed, wg8, rl, sh_saved) if keep else None)


def moe_backward(moe, arena, saved, dout, wg):
    """d(h) [T, d] of ``moe_forward``."""
    h, r, wg8, rl, sh_saved = saved
    E = moe.num_experts
    drl = K.gemm(L.GEMM_NN, dout, moe.up_proj.weight.detach())
    ops._wgrad(arena, moe.up_proj.weight, None, dout, rl, wg)
    dx_lat, dw = ops_moe.routed_backward(_experts(moe, arena), r, drl, wg)
    dh = K.gemm(L.GEMM_NN, dx_lat, moe.down_proj.weight.detach())
    ops._wgrad(arena, moe.down_proj.weight, None, dx_lat, h, wg)
    dlog = ops_moe.gate_buffer(h.shape[0], E, h.device)
    KL.route_bwd(dw, r.s, r.idx, r.p, float(moe.routed_scaling_factor), dlogits=dlog[:, :E])
    ops_moe.gate_backward(moe.gate, E, arena, h, wg8, dlog, dh, wg)
    return expert_backward(moe.shared_expert, arena, h, sh_saved, dout, wg, dh)


def _expert_node_forward(ex, arena, h, keep):
    y, saved = expert_forward(ex, arena, h)
    return y, ((h, saved) if keep else None)


LatentMoEFn = ops_moe.single_output_node("LatentMoEFn", moe_forward, moe_backward, ops.arena_for, ops._flush_wgrads)  # ``LatentMoE.forward`` on [..., d] bf16
ExpertFn = ops_moe.single_output_node(  # ``Expert.forward`` called on its own
    "Expert", _expert_node_forward, lambda ex, arena, saved, dy, wg: expert_backward(ex, arena, *saved, dy, wg), ops.arena_for, ops._flush_wgrads)


def run_moe(moe, x):
    ops_moe._check(moe, x, "LatentMoE")
    b = moe.biases
    if not b.is_cuda or b.dtype not in (BF16, F32):
        raise TypeError(f"LatentMoE: the balancing biases must be a bf16 or fp32 buffer on the GPU, got {b.dtype} on {b.device}")
    return LatentMoEFn.apply(x, moe, torch.is_grad_enabled(), *_param_list(moe))


def run_expert(ex, x):
    ops_moe._check(ex, x, "Expert")
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
