"""Qwen3 mixture-of-experts layer on HIP kernels -- API of ``llm_quest/moe/qwen3_moe.py`` (router_weights_init, Expert, Qwen3MoE).

The layer runs as ONE autograd node (``ops_moe.MoEFn``; inside ``MoETransformerBlock`` the whole block is one): the router, the
token-to-expert plan, the row dispatch and the weighted combine are ``csrc/moe.hip``, the expert products segmented GEMMs (``csrc/gemm_segmented.hip``): one launch
per product over all experts, the segment table read on the device -- no host read.  bf16 training path and no-grad forward.

Differences from upstream, all refusals or definitions where upstream leaves a gap:
  * only SiLU experts; ``shared_expert_hidden_dim`` (the Qwen3-Next shared expert) raises ``NotImplementedError``;
  * ``num_experts`` must be a multiple of 8, at most 128 (the gate's matrix products move 16-byte rows), ``top_k`` at most 8;
  * an expert that received no token ends the step with an exactly zero gradient (upstream: ``grad = None``);
  * among equal bf16 probabilities the lower expert index is selected (``torch.topk`` promises no order there);
  * the returned gate probabilities are not differentiable.
"""

import torch
import torch.nn as nn

from llm_quest_amd import kernels_moe as KM
from llm_quest_amd import ops_moe


def router_weights_init(weights):
    """Re-initialise router / gate weights following the sigma-MoE initialisation used in Qwen3-Next (https://arxiv.org/abs/2310.10837):
    rows of unit L2 norm, rescaled to the original standard deviation (reference: qwen3_moe.py:15-35).  One-time set-up, plain torch."""
    with torch.no_grad():
        og_std = weights.std()
        l2_norms = torch.linalg.vector_norm(weights, dim=-1, ord=2, keepdim=True)
        weights *= l2_norms.reciprocal()
        weights *= og_std / weights.std()


class Expert(nn.Module):
    """lin2(lin1(x) * silu(lin_gate(x))), no biases (reference: qwen3_moe.py:38-66).  On its own it is the dense SwiGLU FFN node."""

    def __init__(self, cfg, hidden_dim=None, activation=torch.nn.functional.silu):
        super().__init__()
        if activation is not torch.nn.functional.silu:
            raise NotImplementedError("Expert: only the SiLU activation has kernels (SwiGLU)")
        self.hidden_dim = hidden_dim if hidden_dim is not None else cfg["moe_hidden_dim"]
        # lin1 then lin_gate: adjacent in the arena -> one [2*hidden, emb] GEMM
        self.lin1 = nn.Linear(cfg["emb_dim"], self.hidden_dim, dtype=cfg["dtype"], bias=False)
        self.activation = activation
        self.lin_gate = nn.Linear(cfg["emb_dim"], self.hidden_dim, dtype=cfg["dtype"], bias=False)
        self.lin2 = nn.Linear(self.hidden_dim, cfg["emb_dim"], dtype=cfg["dtype"], bias=False)

    def forward(self, x):
        from llm_quest_amd import _lib as L
        from llm_quest_amd.qwen.qwen3.qwen3_transformer_block import _FFNFn

        L.require_gpu(x)
        if not hasattr(self, "_param_list"):
            object.__setattr__(self, "_param_list", list(self.parameters()))
        return _FFNFn.apply(x, self, torch.is_grad_enabled(), *self._param_list)


class Qwen3MoE(nn.Module):
    """Sparse mixture of experts: a gate selects ``top_k`` of ``num_experts`` SwiGLU experts per token, their outputs are combined with the
    renormalised gate probabilities (reference: qwen3_moe.py:69-167).  ``moe_loss`` (the load-balancing loss) is set in training mode only."""

    def __init__(self, cfg):
        super().__init__()
        self.top_k = cfg["top_k"]
        self.num_experts = cfg["num_experts"]
        self.load_coeff = cfg["aux_loss_coef"]
        self.re_init_router_weights = cfg.get("re_init_router_weights", False)
        self.shared_expert_hidden_dim = cfg.get("shared_expert_hidden_dim", None)
        if self.shared_expert_hidden_dim is not None:
            raise NotImplementedError("Qwen3MoE: 'shared_expert_hidden_dim' (the Qwen3-Next weighted shared expert) has no kernels here yet")
        KM.check_route(0, self.num_experts, self.top_k)
        if self.num_experts % 8 or cfg["emb_dim"] % 8 or cfg["moe_hidden_dim"] % 8:
            raise ValueError(f"Qwen3MoE: num_experts ({self.num_experts}), emb_dim and moe_hidden_dim must be multiples of 8 (16-byte rows)")
        self.experts = nn.ModuleList([Expert(cfg) for _ in range(cfg["num_experts"])])
        self.gate = nn.Linear(cfg["emb_dim"], cfg["num_experts"], bias=False, dtype=cfg["dtype"])

    def forward(self, x, gate_probas=None, return_gate_probas=False):
        if gate_probas is not None and gate_probas.dim() != 2:
            raise ValueError("gate_probas must be 2D shaped as (batch*seq, num_experts)")
        out, loss, probas = ops_moe.run_moe(self, x, gate_probas)
        if self.training:
            self.moe_loss = loss
        return (out, probas) if return_gate_probas else out
