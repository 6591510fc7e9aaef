"""Nemotron-3 LatentMoE on HIP kernels -- API of ``llm_quest/moe/nvidia_latent_moe.py`` (SquaredReLU, Expert, LatentMoE).

The layer runs as ONE autograd node (``ops_latmoe.LatentMoEFn``): a down projection to ``emb_dim // latent_ratio``, ``latent_ratio`` times as many routed
experts and ``latent_ratio`` times the ``top_k`` working at that latent width, the routed sum accumulated in the latent space, one up projection and
one full-width shared expert.  The sigmoid router (balancing biases, ``routed_scaling_factor``), its backward and the squared-ReLU GLU of every expert are
``csrc/latent_moe.hip``; the token-to-expert plan, the row dispatch and the combine are ``csrc/moe.hip``, the bias update ``csrc/deepseek_moe.hip``; the
routed experts' products are segmented GEMMs (``csrc/gemm_segmented.hip``: one launch per product over all routed experts, no host read), the gate's,
the projections' and the shared expert's the existing GEMMs.  bf16 training path and no-grad forward.  ``state_dict`` matches upstream key for key;
``biases`` is an fp32 buffer after plain construction (an fp32 selection key, an fp32 update) and bf16 after ``.to(bfloat16)`` -- both run.

As upstream, ``routed_expert_hidden_dim`` is stored and the routed experts are built with ``cfg["moe_hidden_dim"]``.

Limits, each a ``ValueError`` of the constructor: ``emb_dim % latent_ratio == 0``; the latent width, ``moe_hidden_dim`` and the shared expert's hidden size
positive multiples of 8 (16-byte rows); 1..128 routed experts; ``top_k`` in 1..8 and at most the number of experts.
Definitions where upstream leaves a gap:
  * among equal selection keys the lower expert index is selected (``torch.topk`` promises no order there);
  * an expert that received no token ends the step with an exactly zero gradient (upstream: ``grad = None``);
  * the bias update runs on the device from the plan's counts, without a host read, and only in training mode, as upstream (``if self.training``);
    ``max_vio`` (an fp32 0-dim tensor, the batch's max violation) is left on the module by every training forward;
  * ``_forced_topk`` (private, as on ``DeepSeekMoE``): an int tensor [tokens, top_k] on the module makes the router skip the selection and weigh the given
    experts with its own probabilities; ``None`` (the default) routes normally;
  * ``Expert`` and ``SquaredReLU`` used on their own run on the same kernels (``SquaredReLU`` as the GLU with u = 1; last dimension a multiple of 8).
    An ``Expert`` built with another ``activation`` has no kernel: its forward raises.
"""

import torch
import torch.nn as nn

from llm_quest_amd import kernels_moe as KM
from llm_quest_amd import ops_latmoe


class SquaredReLU(nn.Module):
    """relu(x)^2 (nvidia_latent_moe.py:5-14; https://arxiv.org/abs/2109.08668), the FFN activation of Nemotron 3."""

    def forward(self, x):
        return ops_latmoe.run_relu2(x)


class Expert(nn.Module):
    """lin2(lin1(x) * activation(lin_gate(x))), no biases, ``input_dim`` -> ``hidden_dim`` -> ``input_dim`` (nvidia_latent_moe.py:17-44).

    Args:
        cfg (dict): Config dictionary containing model hyperparameters.
        input_dim (int): Input dimension of the expert. If None, will use the emb_dim from the config.
        hidden_dim (int): Hidden dimension of the expert. If None, will use the moe_hidden_dim from the config.
        activation: activation module class; only SquaredReLU has kernels
    """

    def __init__(self, cfg, input_dim=None, hidden_dim=None, activation=SquaredReLU):
        super().__init__()
        self.hidden_dim = hidden_dim if hidden_dim is not None else cfg["moe_hidden_dim"]
        self.input_dim = input_dim if input_dim is not None else cfg["emb_dim"]
        _check_width("Expert", "input_dim", self.input_dim)
        _check_width("Expert", "hidden_dim", self.hidden_dim)

        self.lin1 = nn.Linear(self.input_dim, self.hidden_dim, dtype=cfg["dtype"], bias=False)
        self.activation = activation()
        self.lin_gate = nn.Linear(self.input_dim, self.hidden_dim, dtype=cfg["dtype"], bias=False)
        self.lin2 = nn.Linear(self.hidden_dim, self.input_dim, dtype=cfg["dtype"], bias=False)

    def forward(self, x):
        if not isinstance(self.activation, SquaredReLU):
            raise NotImplementedError(f"Expert: only the SquaredReLU activation has kernels, got {type(self.activation).__name__}")
        return ops_latmoe.run_expert(self, x)


def _check_width(who, name, n):
    if not isinstance(n, int) or n <= 0 or n % 8:
        raise ValueError(f"{who}: {name} must be a positive multiple of 8 (16-byte rows), got {n}")


class LatentMoE(nn.Module):
    """Nvidia LatentMoE (nvidia_latent_moe.py:47-135; https://research.nvidia.com/labs/nemotron/files/NVIDIA-Nemotron-3-White-Paper.pdf): DeepSeek's
    auxiliary-loss-free balanced routing on a sigmoid gate, with a single shared expert, latent projection layers around the routed experts and a latent
    ratio that scales the number of experts and ``top_k``."""

    def __init__(
        self,
        cfg,
        top_k=2,
        num_experts=4,
        routed_expert_hidden_dim=None,
        shared_expert_hidden_dim=None,
        routed_scaling_factor=2.5,  # increase signal/scale up for gradient (unrelated to LatentMoE)
        latent_ratio=4,  # emb_dim / latent_dim (default to 4 per Nvidia Nemotron 3)
        bias_update_rate=1e-3,  # aux-loss free load balancing rate
    ):
        super().__init__()
        # the experts are scaled up by latent_ratio, in case it's not already done in the config
        self.top_k = cfg.get("top_k", top_k * latent_ratio)
        self.num_experts = cfg.get("num_experts", num_experts * latent_ratio)

        if not isinstance(latent_ratio, int) or latent_ratio <= 0 or cfg["emb_dim"] % latent_ratio:
            raise ValueError(f"LatentMoE: emb_dim ({cfg['emb_dim']}) must be divisible by latent_ratio ({latent_ratio})")
        self.latent_dim = cfg["emb_dim"] // latent_ratio
        self.routed_scaling_factor = cfg.get("routed_scaling_factor", routed_scaling_factor)
        self.shared_expert_hidden_dim = cfg.get("shared_expert_hidden_dim", shared_expert_hidden_dim)
        self.routed_expert_hidden_dim = cfg.get("routed_expert_hidden_dim", routed_expert_hidden_dim)

        # the kernels' limits
        _check_width("LatentMoE", "the latent width emb_dim // latent_ratio", self.latent_dim)
        _check_width("LatentMoE", "moe_hidden_dim", cfg["moe_hidden_dim"])
        _check_width("LatentMoE", "the shared expert's hidden size",
                     self.shared_expert_hidden_dim if self.shared_expert_hidden_dim is not None else cfg["moe_hidden_dim"])
        KM.check_route(0, self.num_experts, self.top_k)

        self.routed_experts = nn.ModuleList([Expert(cfg, input_dim=self.latent_dim) for _ in range(self.num_experts)])
        self.shared_expert = Expert(cfg, hidden_dim=self.shared_expert_hidden_dim)
        self.gate = nn.Linear(cfg["emb_dim"], self.num_experts, bias=False, dtype=cfg["dtype"])

        # bias for Aux-Loss free load balancing
        self.register_buffer("biases", torch.zeros(self.num_experts))
        self.bias_update_rate = bias_update_rate

        # latent projection layers
        self.down_proj = nn.Linear(cfg["emb_dim"], self.latent_dim, bias=False, dtype=cfg["dtype"])
        self.up_proj = nn.Linear(self.latent_dim, cfg["emb_dim"], bias=False, dtype=cfg["dtype"])
        self._forced_topk = None

    def forward(self, x):
        return ops_latmoe.run_moe(self, x)
