"""Classic mixture of experts on HIP kernels -- API of ``llm_quest/moe/classic_moe.py`` (ExpertGeLU, MoE, MoE_old).

The layer runs as ONE autograd node (``ops_cmoe.MoEFn``): a softmax gate with a bias, the ``top_k`` largest probabilities renormalised, GPT-2-style experts
(Linear + bias -> erf GELU -> Linear + bias, hidden size ``int(4 * scaling_factor * emb_dim)``) and the loss
``moe_loss = z_router_coeff * mean(logsumexp(logits)^2) + load_coeff * num_experts * <f, p>``, left on the module by EVERY forward as a differentiable
0-dim tensor of the activation dtype.  The router (with the z-loss's logsumexp), its backward, the loss, the experts' bias + GELU passes over the
expert-sorted buffer and the biases' gradients are ``csrc/classic_moe.hip``; the token-to-expert plan, the row dispatch and the combine are
``csrc/moe.hip``; the experts' products are segmented GEMMs (``csrc/gemm_segmented.hip``: one launch per product over all experts, no host read).
bf16 parameters and activations on the GPU only (upstream after ``.to(torch.bfloat16)``); training path and no-grad forward.  ``state_dict`` matches
upstream key for key.

``MoE_old`` is upstream's unoptimised forward of the same function (one masked pass per expert instead of ``index_add_`` per hit expert); here it is a
thin subclass that runs the same node.

Limits, each a ``ValueError`` of the constructor naming the argument: ``emb_dim`` and the experts' ``hidden_dim`` positive multiples of 8 (16-byte
rows); ``num_experts`` at most 128; ``top_k`` at most 8.  The two assertions are upstream's.
Definitions where upstream leaves a gap:
  * among equal probabilities the lower expert index is selected (``torch.topk`` promises no order there);
  * an expert that received no token ends the step with an exactly zero gradient (upstream: ``grad = None``);
  * ``_forced_topk`` (private, as on ``DeepSeekMoE``): an int tensor [tokens, top_k] on the module makes the router skip the selection and weigh the given
    experts with its own probabilities; ``None`` (the default) routes normally;
  * ``ExpertGeLU`` used on its own is the dense FFN on the GEMM's bias / GELU epilogues, with autograd.
"""

import torch.nn as nn

from llm_quest_amd import ops_cmoe


def _check_width(who, name, n):
    if not isinstance(n, int) or n <= 0 or n % 8:
        raise ValueError(f"{who}: {name} must be a positive multiple of 8 (16-byte rows), got {n}")


class ExpertGeLU(nn.Module):
    """A single expert (classic_moe.py:7-30): the GPT-2 FFN with a modular hidden size.

    Args:
        cfg (dict): Config dictionary containing model hyperparameters. It must include the "emb_dim".
        scaling_factor (float): A multiplier used to scale the hidden layer size.
    """

    def __init__(self, cfg, scaling_factor):
        super().__init__()
        self.hidden_dim = int(4 * scaling_factor * cfg["emb_dim"])
        _check_width("ExpertGeLU", "emb_dim", cfg["emb_dim"])
        _check_width("ExpertGeLU", "hidden_dim = int(4 * scaling_factor * emb_dim)", self.hidden_dim)

        self.layers = nn.Sequential(
            nn.Linear(cfg["emb_dim"], self.hidden_dim),
            nn.GELU(),
            nn.Linear(self.hidden_dim, cfg["emb_dim"]),
        )

    def forward(self, x):
        return ops_cmoe.run_expert(self, x)


class MoE(nn.Module):
    """Mixture of Experts layer (classic_moe.py:33-125): a gate selects ``top_k`` experts per token, their outputs are combined with the renormalised
    probabilities.

    Args:
        cfg (dict): Config dictionary containing model hyperparameters. It must include "emb_dim".
        num_experts (int): Total number of experts.
        top_k (int): Number of experts to select
        scaling_factor (float or "auto"): Scaling factor for the hidden layer size of each expert; "auto" = 1 / top_k (the active experts together
            match the GPT-2 FFN size)
        load_coeff (float): Coefficient for the load balancing loss.
        z_router_coeff (float): Coefficient for the router z-loss.

    Attributes:
        moe_loss (torch.Tensor): Total moe loss, combining load balancing and router z-loss.
    """

    def __init__(
        self,
        cfg,
        num_experts=8,
        top_k=2,
        scaling_factor="auto",
        load_coeff=10e-2,
        z_router_coeff=1e-3,
    ):
        super().__init__()
        assert (scaling_factor == "auto") or (
            cfg["emb_dim"] % scaling_factor == 0
        ), "emb_dim must be divisible by scaling_factor"
        assert 0 < top_k <= num_experts, "top_k must be > 0 and and <= num_experts"
        # the kernels' limits
        if num_experts > 128:
            raise ValueError(f"MoE: num_experts must be at most 128, got {num_experts}")
        if top_k > 8:
            raise ValueError(f"MoE: top_k must be at most 8, got {top_k}")

        if scaling_factor == "auto":
            scaling_factor = 1 / top_k
        self.experts = nn.ModuleList([ExpertGeLU(cfg, scaling_factor) for _ in range(num_experts)])
        self.gate = nn.Linear(cfg["emb_dim"], num_experts, bias=True)
        self.top_k = top_k
        self.num_experts = num_experts
        self.load_coeff = load_coeff
        self.z_router_coeff = z_router_coeff
        self._forced_topk = None

    def forward(self, x):
        out, self.moe_loss = ops_cmoe.run_moe(self, x)
        return out


class MoE_old(MoE):
    """Upstream's original, unoptimised forward (classic_moe.py:129-217) computes the same function as ``MoE``: the same constructor, the same node."""
