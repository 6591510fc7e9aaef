"""Gemma3 RMSNorm, GELU, GeGLU FFN and transformer block -- API of ``llm_quest/llama3_to_gemma3/gemma3_transformer_block.py``."""

import torch
import torch.nn as nn

from llm_quest_amd import kernels as K
from llm_quest_amd import ops_g3
from llm_quest_amd.llama3_to_gemma3.gemma3_attention import GroupedQueryAttention


class RMSNorm(nn.Module):
    """scale * x / (RMS(x) + eps): eps is added to the RMS, not under the root (gemma3_transformer_block.py:14-37)."""

    def __init__(self, emb_dim, dtype=None):
        super().__init__()
        self.eps = 1e-6
        self.scale = nn.Parameter(torch.ones(emb_dim, dtype=dtype))

    def forward(self, x):
        ops_g3._check_activation(x, "RMSNorm")
        ops_g3.check_bf16(self, "RMSNorm")
        return ops_g3.RMSNormFn.apply(x, self, self.scale)


class _GeluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x2 = x if x.is_contiguous() else x.contiguous()
        ctx.x = x2
        return K.gelu_fwd(x2)

    @staticmethod
    def backward(ctx, dy):
        return K.gelu_bwd(ctx.x, dy if dy.is_contiguous() else dy.contiguous())


class GELU(nn.Module):
    """x * Phi(x) with the error function (gemma3_transformer_block.py:40-58)."""

    def __init__(self):
        super().__init__()

    def forward(self, x):
        ops_g3._check_activation(x, "GELU")
        return _GeluFn.apply(x)


class FFN(nn.Module):
    """lin2(lin1(x) * gelu(lin_gate(x))), no biases (gemma3_transformer_block.py:61-106)."""

    def __init__(self, cfg):
        super().__init__()
        # lin1 then lin_gate: adjacent in the arena -> one [2 * hidden, emb] GEMM
        self.lin1 = nn.Linear(cfg["emb_dim"], cfg["hidden_dim"], dtype=cfg["dtype"], bias=False)
        self.lin_gate = nn.Linear(cfg["emb_dim"], cfg["hidden_dim"], dtype=cfg["dtype"], bias=False)
        self.gelu_activ = GELU()
        self.lin2 = nn.Linear(cfg["hidden_dim"], cfg["emb_dim"], dtype=cfg["dtype"], bias=False)

    def forward(self, x):
        ops_g3._check_activation(x, "FFN")
        ops_g3.check_bf16(self, "FFN")
        return ops_g3.FFNFn.apply(x, self, torch.is_grad_enabled(), *ops_g3._param_list(self))


class TransformerBlock(nn.Module):
    """x + post_att_norm(att(pre_att_norm(x))); x + post_ffn_norm(ffn(pre_ffn_norm(x))) (gemma3_transformer_block.py:109-162).

    Runs as ONE autograd node (ops_g3.Gemma3BlockFn); the residual adds ride on the post-norm kernels and on the norm backwards."""

    def __init__(self, cfg, layer):
        super().__init__()
        self.att = GroupedQueryAttention(
            d_in=cfg["emb_dim"], d_out=cfg["emb_dim"], num_heads=cfg["n_heads"], num_kv_groups=cfg["num_kv_groups"], window_size=cfg["window_size"],
            layer_id=layer, dtype=cfg["dtype"], local_global_att_ratio=cfg["local_global_att_ratio"],
        )
        self.pre_att_norm = RMSNorm(cfg["emb_dim"])
        self.post_att_norm = RMSNorm(cfg["emb_dim"])
        self.pre_ffn_norm = RMSNorm(cfg["emb_dim"])
        self.post_ffn_norm = RMSNorm(cfg["emb_dim"])
        self.ffn = FFN(cfg)

    def forward(self, x, mask, cos, sin, swa_mask=None, _runtime=None):
        B, S, _ = x.shape
        rt = _runtime if _runtime is not None else ops_g3.make_runtime(self, B, S, cos, sin)
        return ops_g3.run_block(self, x, rt)
