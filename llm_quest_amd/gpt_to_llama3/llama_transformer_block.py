"""Llama 3.2 RMSNorm, SiLU, SwiGLU FFN and the transformer block -- API of ``llm_quest/gpt_to_llama3/llama_transformer_block.py``."""

import torch
import torch.nn as nn

from llm_quest_amd import ops_g3, ops_llama
from llm_quest_amd.gpt_to_llama3.llama_attention import GroupedQueryAttention


class RMSNorm(nn.Module):
    """scale * x / (RMS(x) + eps): eps is added to the RMS, the normalisation runs in fp32 and is rounded before the scale multiplies it
    (llama_transformer_block.py:15-38) -- the form ``mi355_g3_rmsnorm_fwd/_bwd`` implement."""

    def __init__(self, emb_dim, dtype=None):
        super().__init__()
        self.eps = 1e-6
        self.scale = nn.Parameter(torch.ones(emb_dim, dtype=dtype))

    def forward(self, x):
        ops_g3._check_activation(x, "RMSNorm")
        ops_llama.check_bf16(self, "RMSNorm")
        return ops_g3.RMSNormFn.apply(x, self, self.scale)


class SiLU(nn.Module):
    """x * sigmoid(x) (llama_transformer_block.py:41-58)."""

    def __init__(self) -> None:
        super().__init__()

    def forward(self, x):
        ops_g3._check_activation(x, "SiLU")
        return ops_llama.SiLUFn.apply(x)


class FFN(nn.Module):
    """lin2(lin1(x) * silu(lin_gate(x))), no biases (llama_transformer_block.py:61-107)."""

    def __init__(self, cfg):
        super().__init__()
        # lin1 then lin_gate: adjacent in the arena -> one [2 * hidden, emb] GEMM
        self.lin1 = nn.Linear(cfg["emb_dim"], cfg["hidden_dim"], dtype=cfg["dtype"], bias=False)
        self.lin_gate = nn.Linear(cfg["emb_dim"], cfg["hidden_dim"], dtype=cfg["dtype"], bias=False)
        self.silu_activ = SiLU()
        self.lin2 = nn.Linear(cfg["hidden_dim"], cfg["emb_dim"], dtype=cfg["dtype"], bias=False)

    def forward(self, x):
        ops_g3._check_activation(x, "FFN")
        ops_llama.check_bf16(self, "FFN")
        return ops_llama.FFNFn.apply(x, self, torch.is_grad_enabled(), *ops_llama._param_list(self))


class TransformerBlock(nn.Module):
    """x + att(norm_1(x)); x + ffn(norm_2(x)) (llama_transformer_block.py:110-154).

    Runs as ONE autograd node (ops_llama.LlamaBlockFn); the residual adds ride on the out-projection and on the lin2 GEMM."""

    def __init__(self, cfg):
        super().__init__()
        self.att = GroupedQueryAttention(
            d_in=cfg["emb_dim"],
            d_out=cfg["emb_dim"],
            num_heads=cfg["n_heads"],
            num_kv_groups=cfg["num_kv_groups"],
            dtype=cfg["dtype"],
        )
        self.norm_1 = RMSNorm(cfg["emb_dim"])
        self.norm_2 = RMSNorm(cfg["emb_dim"])
        self.ffn = FFN(cfg)

    def forward(self, x, mask, cos, sin, attn_mask=None, _runtime=None):
        B, S, _ = x.shape
        rt = _runtime if _runtime is not None else ops_llama.make_runtime(self, B, S, cos, sin, attn_mask)
        return ops_llama.run_block(self, x, rt)
