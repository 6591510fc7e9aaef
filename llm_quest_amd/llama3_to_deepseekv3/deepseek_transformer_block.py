"""DeepSeek-V3 RMSNorm, SiLU, SwiGLU FFN and the dense transformer block -- API of
``llm_quest/llama3_to_deepseekv3/deepseek_transformer_block.py``.  Layers ``layer >= cfg["num_ffn"]`` hold a ``DeepSeekMoE`` (``moe/deepseek_moe.py``)."""

import torch
import torch.nn as nn

from llm_quest_amd import ops_dsmoe, ops_g3, ops_mla
from llm_quest_amd.llama3_to_deepseekv3.deepseek_attention import MultiLatentAttention, RMSNorm  # noqa: F401  (RMSNorm: same class upstream defines here)
from llm_quest_amd.moe.deepseek_moe import DeepSeekMoE


class SiLU(nn.Module):
    """x * sigmoid(x) (deepseek_transformer_block.py:41-58)."""

    def __init__(self) -> None:
        super().__init__()

    def forward(self, x):
        ops_g3._check_activation(x, "SiLU")
        return ops_mla.SiLUFn.apply(x)


class FFN(nn.Module):
    """lin2(lin1(x) * silu(lin_gate(x))), no biases (deepseek_transformer_block.py:61-107)."""

    def __init__(self, cfg):
        super().__init__()
        # lin1 then lin_gate: adjacent in the arena -> one [2 * hidden, emb] GEMM
        self.lin1 = nn.Linear(cfg["emb_dim"], cfg["hidden_dim"], dtype=cfg["dtype"], bias=False)
        self.lin_gate = nn.Linear(cfg["emb_dim"], cfg["hidden_dim"], dtype=cfg["dtype"], bias=False)
        self.silu_activ = SiLU()
        self.lin2 = nn.Linear(cfg["hidden_dim"], cfg["emb_dim"], dtype=cfg["dtype"], bias=False)

    def forward(self, x):
        ops_g3._check_activation(x, "FFN")
        ops_g3.check_bf16(self, "FFN")
        return ops_mla.FFNFn.apply(x, self, torch.is_grad_enabled(), *ops_mla._param_list(self))


class TransformerBlock(nn.Module):
    """x + att(norm_1(x)); x + ffn(norm_2(x)) (deepseek_transformer_block.py:110-155): ``ffn`` is the dense ``FFN`` for ``layer < cfg["num_ffn"]`` and a
    ``DeepSeekMoE`` from there on (a config without the MoE keys is refused there with ``NotImplementedError``).

    Runs as ONE autograd node (ops_mla.DeepSeekBlockFn / ops_dsmoe.DeepSeekMoEBlockFn); the residual adds ride on the out-projection and on the lin2
    GEMM, resp. the MoE combine."""

    def __init__(self, cfg, layer):
        super().__init__()
        self.att = MultiLatentAttention(
            d_in=cfg["emb_dim"],
            d_out=cfg["emb_dim"],
            num_heads=cfg["n_heads"],
        )
        self.norm_1 = RMSNorm(cfg["emb_dim"])
        self.norm_2 = RMSNorm(cfg["emb_dim"])
        self.ffn = FFN(cfg) if layer < cfg["num_ffn"] else DeepSeekMoE(cfg)

    def forward(self, x, mask, cos, sin, _runtime=None):
        B, S, _ = x.shape
        ops_mla.check_mask(mask, S)
        rt = _runtime if _runtime is not None else ops_mla.make_runtime(self, B, S, cos, sin)
        if isinstance(self.ffn, DeepSeekMoE):
            return ops_dsmoe.run_block(self, x, rt)
        return ops_mla.run_block(self, x, rt)
