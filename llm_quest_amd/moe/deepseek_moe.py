"""DeepSeekMoE on HIP kernels -- API of ``llm_quest/moe/deepseek_moe.py`` (Expert, VectorizedLinear, VectorizedSharedExperts, DeepSeekMoE,
max_violation_batch, max_violation_step).

The layer runs as ONE autograd node (``ops_dsmoe.DeepSeekMoEFn``; inside the DeepSeek-V3 ``TransformerBlock`` the whole block is one): the
bias-balanced router, the bias update, the shared experts' bias + SiLU and the combine are ``csrc/deepseek_moe.hip``; the token-to-expert plan, the
row dispatch and the backwards of combine and router are ``csrc/moe.hip``; the routed experts' products are segmented GEMMs (``csrc/gemm_segmented.hip``: one launch per
product over all routed experts, no host read), the gate's and the shared experts' the existing GEMMs.  bf16 training path and no-grad
forward.  ``state_dict`` matches upstream key for key.

Limits, checked in the constructor: 1..128 routed experts (any value), ``top_k`` at most 8, ``emb_dim`` and the scaled hidden size multiples of 8.
Definitions where upstream leaves a gap, and deviations:
  * among equal selection keys the lower expert index is selected (``torch.topk`` promises no order there);
  * an expert that received no token ends the step with an exactly zero gradient (upstream: ``grad = None``);
  * ``max_vio`` and the bias update are computed on the device from the plan's counts, without a host read; ``max_vio`` is an fp32 0-dim tensor;
  * ``max_violation_step`` returns the mean of ``ffn.max_vio`` over the blocks that have one (upstream's cannot run: it hands ``hasattr`` a float).
``_forced_topk`` (private, in the spirit of ``_runtime``): an int tensor [tokens, top_k] on the module makes the router skip the selection and
weigh the given experts with its own probabilities; ``None`` (the default) routes normally.
"""

import math

import torch
import torch.nn as nn

from llm_quest_amd import kernels_moe as KM
from llm_quest_amd import ops_dsmoe, ops_mla, ops_moe

MOE_KEYS = ("num_experts", "num_shared_experts", "top_k", "moe_scaling_factor", "moe_bias_update_rate")


def _scaled_hidden(cfg, scaling_factor):
    return int(scaling_factor * cfg["hidden_dim"])


class Expert(nn.Module):
    """lin2(silu(lin1(x)) * lin_gate(x)), no biases, hidden size ``int(scaling_factor * cfg["hidden_dim"])`` (deepseek_moe.py:9-35).  The SiLU sits
    on ``lin1`` (the dense ``FFN`` and ``Qwen3MoE.Expert`` put it on ``lin_gate``).  On its own it is the SwiGLU FFN node with the halves exchanged."""

    def __init__(self, cfg, scaling_factor):
        super().__init__()
        self.hidden_dim = _scaled_hidden(cfg, scaling_factor)

        self.lin1 = nn.Linear(cfg["emb_dim"], self.hidden_dim, dtype=cfg["dtype"], bias=False)
        self.lin_gate = nn.Linear(cfg["emb_dim"], self.hidden_dim, dtype=cfg["dtype"], bias=False)
        self.lin2 = nn.Linear(self.hidden_dim, cfg["emb_dim"], dtype=cfg["dtype"], bias=False)

    def forward(self, x):
        return _ExpertFn.apply(x, self, torch.is_grad_enabled(), *_checked(self, x, "Expert"))


def _checked(module, x, what):
    ops_moe._check(module, x, what)
    return ops_mla._param_list(module)


class _Halves:
    """The view of an ``Expert`` that ``ops_mla.ffn_forward`` / ``ffn_backward`` take: their u * silu(g) with u = lin_gate, g = lin1."""

    def __init__(self, ex):
        self.lin1, self.lin_gate, self.lin2 = ex.lin_gate, ex.lin1, ex.lin2


class _ExpertFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ex, keep, *params):
        arena = ops_dsmoe.ensure_arena(_as_routed(ex))
        x2 = ops_mla._flat(x)
        y, saved = ops_mla.ffn_forward(_Halves(ex), arena, x2)
        ctx.ex, ctx.shape, ctx.saved = ex, x.shape, ((x2, saved) if keep else None)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        if ctx.saved is None:
            raise RuntimeError("Expert: backward through a forward that ran without grad mode")
        x2, saved = ctx.saved
        dx = ops_mla.ffn_backward(_Halves(ctx.ex), ops_dsmoe.ensure_arena(ctx.ex), x2, saved, ops_mla._flat(dy))
        ctx.saved = None
        return (dx.view(ctx.shape), None, None) + (None,) * len(ctx.ex._param_list)


def _as_routed(ex):
    """An Expert used on its own gets an arena with lin_gate in front of lin1, as inside the layer."""
    if getattr(ex, "_arena", None) is None:
        from llm_quest_amd.arena import ParamArena

        ar = ParamArena([("lin_gate.weight", ex.lin_gate.weight), ("lin1.weight", ex.lin1.weight), ("lin2.weight", ex.lin2.weight)])
        for m in ex.modules():
            object.__setattr__(m, "_arena", ar)
    return ex


class VectorizedLinear(nn.Module):
    """A batch of ``num_experts`` linear layers: weight [num_experts, in, out], bias [num_experts, out] (deepseek_moe.py:38-88).  Parameter
    container with upstream's initialisation; the products run inside ``VectorizedSharedExperts``."""

    def __init__(self, num_experts, in_features, out_features, bias=True):
        super().__init__()
        self.num_experts = num_experts
        self.weight = nn.Parameter(torch.empty(num_experts, in_features, out_features))

        if bias:
            self.bias = nn.Parameter(torch.empty(num_experts, out_features))
        else:
            self.bias = None

        self._kaiming_init()

    def _kaiming_init(self):
        """As nn.Linear initialises each of the batch's layers (deepseek_moe.py:63-74).  One-time set-up, plain torch."""
        with torch.no_grad():
            for i in range(self.num_experts):
                nn.init.kaiming_uniform_(self.weight[i], a=math.sqrt(5))
                if self.bias is not None:
                    fan_in, _ = nn.init._calculate_fan_in_and_fan_out(self.weight[i])
                    bound = 1 / math.sqrt(fan_in) if fan_in > 0 else 0
                    nn.init.uniform_(self.bias[i], -bound, bound)

    def forward(self, x):
        raise NotImplementedError("VectorizedLinear holds parameters only; its products run fused inside VectorizedSharedExperts.forward")


class VectorizedSharedExperts(nn.Module):
    """sum_n lin2_n(silu(lin1_n(x))) over ``num_experts`` always-active biased MLPs (deepseek_moe.py:91-129): ``num_experts`` NN GEMMs into the column
    blocks of one [tokens, n * hidden] buffer, the fused bias + SiLU kernel, then ONE NN GEMM with K = n * hidden that is the second product and the
    sum over the experts, the summed ``lin2`` biases riding on it."""

    def __init__(self, num_experts, cfg, scaling_factor, bias=True):
        super().__init__()
        self.hidden_dim = _scaled_hidden(cfg, scaling_factor)
        if self.hidden_dim <= 0 or self.hidden_dim % 8 or cfg["emb_dim"] % 8:
            raise ValueError(f"VectorizedSharedExperts: emb_dim ({cfg['emb_dim']}) and the scaled hidden size ({self.hidden_dim}) must be multiples of 8 (16-byte rows)")
        self.lin1 = VectorizedLinear(num_experts, cfg["emb_dim"], self.hidden_dim, bias)
        self.silu = nn.functional.silu
        self.lin2 = VectorizedLinear(num_experts, self.hidden_dim, cfg["emb_dim"], bias)

    def forward(self, x):
        assert x.ndim == 3, "x should be (b, s, emb_dim)"
        return ops_dsmoe.run_shared(self, x)


class DeepSeekMoE(nn.Module):
    """Shared + routed experts with auxiliary-loss-free load balancing (deepseek_moe.py:132-214): a biased gate selects ``top_k`` of the routed
    experts on ``softmax + biases`` and weighs them with the renormalised unbiased probabilities; after every forward ``biases`` moves by
    ``bias_update_rate * sign(mean(counts) - counts)`` and ``max_vio`` holds the batch's max violation."""

    def __init__(self, cfg):
        super().__init__()
        missing = [key for key in MOE_KEYS if key not in cfg]
        if missing:
            raise NotImplementedError(f"DeepSeekMoE: the config lacks the keys {missing}; a DeepSeekMoE layer needs {list(MOE_KEYS)}")
        num_experts = cfg["num_experts"]
        num_shared_experts = cfg["num_shared_experts"]
        top_k = cfg["top_k"]
        scaling_factor = cfg["moe_scaling_factor"]
        bias_update_rate = cfg["moe_bias_update_rate"]

        # upstream's checks
        if scaling_factor == "auto" or scaling_factor != 1:
            assert (top_k + num_shared_experts) % 2 == 0, (
                f"Total 'active' experts: ({top_k} routed + {num_shared_experts} shared) must be even "
                "for better hidden_dim alignment when scaling_factor != 1"
            )
        assert 0 < top_k <= num_experts - num_shared_experts, "top_k must be > 0 and <= routed experts"

        if scaling_factor == "auto":
            scaling_factor = 1 / (top_k + num_shared_experts)
        self.top_k = top_k
        self.num_experts = num_experts
        self.num_shared = num_shared_experts
        self.num_routed = num_experts - num_shared_experts

        # the kernels' limits
        KM.check_route(0, self.num_routed, top_k)
        hidden = _scaled_hidden(cfg, scaling_factor)
        if hidden <= 0 or hidden % 8 or cfg["emb_dim"] % 8:
            raise ValueError(f"DeepSeekMoE: emb_dim ({cfg['emb_dim']}) and the scaled hidden size ({hidden}) must be multiples of 8 (16-byte rows)")
        if self.num_shared < 0:
            raise ValueError(f"DeepSeekMoE: num_shared_experts must not be negative, got {self.num_shared}")

        self.routed_experts = nn.ModuleList([Expert(cfg, scaling_factor) for _ in range(self.num_routed)])
        if self.num_shared > 0:
            self.shared_experts = VectorizedSharedExperts(self.num_shared, cfg, scaling_factor)

        # gate and balancing biases for the routed experts only
        self.gate = nn.Linear(cfg["emb_dim"], self.num_routed, bias=True)
        self.register_buffer("biases", torch.zeros(self.num_routed))
        self.bias_update_rate = bias_update_rate
        self._forced_topk = None

    def forward(self, x):
        return ops_dsmoe.run_moe(self, x)


def max_violation_batch(load):
    """max-violation of a batch = (max(load) - mean(load)) / mean(load), ``load`` the tokens dispatched to each expert (deepseek_moe.py:218-229).
    A metric helper on a handful of numbers, plain torch; the layer's own ``max_vio`` comes from ``mi355_dsmoe_bias_update``."""
    mean_vio = load.mean()
    max_vio = (load.max() - mean_vio) / mean_vio
    return max_vio


def max_violation_step(model=None):
    """The mean of ``ffn.max_vio`` over the blocks of ``model`` whose ``ffn`` has one (deepseek_moe.py:232-244, made runnable)."""
    max_vios, num_layers = 0.0, 0
    for module in model.modules():
        ffn = getattr(module, "ffn", None)
        if ffn is not None and hasattr(ffn, "max_vio"):
            max_vios = max_vios + ffn.max_vio
            num_layers += 1

    return max_vios / num_layers
