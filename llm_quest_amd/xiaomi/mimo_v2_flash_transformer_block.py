"""MiMo-V2-Flash FFN and transformer block -- API of ``llm_quest/xiaomi/mimo_v2_flash_transformer_block.py``."""

import torch
import torch.nn as nn

from llm_quest_amd import ops_g3, ops_mimo, ops_mla
from llm_quest_amd.moe.deepseek_moe import DeepSeekMoE
from llm_quest_amd.qwen.qwen3.qwen3_attention import PytorchRMSNorm
from llm_quest_amd.xiaomi.mimo_v2_flash_attention import GroupedQueryAttentionWithSink


class FFN(nn.Module):
    """lin2(lin1(x) * silu(lin_gate(x))), no biases (mimo_v2_flash_transformer_block.py:8-22), on the fused gate-up kernels."""

    def __init__(self, cfg):
        super().__init__()
        # lin1 then lin_gate: adjacent in the arena -> one [2 * hidden, emb] GEMM
        self.lin1 = nn.Linear(cfg["emb_dim"], cfg["hidden_dim"], dtype=cfg["dtype"], bias=False)
        self.lin_gate = nn.Linear(cfg["emb_dim"], cfg["hidden_dim"], dtype=cfg["dtype"], bias=False)
        self.silu_activ = nn.functional.silu
        self.lin2 = nn.Linear(cfg["hidden_dim"], cfg["emb_dim"], dtype=cfg["dtype"], bias=False)

    def forward(self, x):
        ops_g3._check_activation(x, "FFN")
        ops_g3.check_bf16(self, "FFN")
        return ops_mla.FFNFn.apply(x, self, torch.is_grad_enabled(), *ops_mla._param_list(self))


class TransformerBlock(nn.Module):
    """x + att(norm1(x)); x + feed_forward(norm2(x)) (mimo_v2_flash_transformer_block.py:25-91): global (causal, ``num_ga_kv_groups``, no sink) or
    sliding-window (``window_size``, ``num_swa_kv_groups``, a sink) attention, and a dense ``FFN`` or a ``DeepSeekMoE`` with 0 shared experts.

    Runs as ONE autograd node (ops_mimo.MiMoBlockFn); the residual adds ride on the out-projection and on the lin2 GEMM, resp. the MoE combine.
    ``mask`` is accepted for API parity and never read: the window is ``cfg["window_size"]``."""

    def __init__(self, cfg, layer_idx, use_sliding_window=True, use_moe=True):
        super().__init__()
        self.layer_idx = layer_idx
        self.use_sliding_window = use_sliding_window
        self.use_moe = use_moe

        if use_sliding_window:
            num_kv_groups = cfg["num_swa_kv_groups"]
        else:
            num_kv_groups = cfg["num_ga_kv_groups"]
        self.window_size = cfg["window_size"] if use_sliding_window else None
        self.context_length = cfg["context_length"]

        self.att = GroupedQueryAttentionWithSink(
            d_in=cfg["emb_dim"],
            num_heads=cfg["n_heads"],
            num_kv_groups=num_kv_groups,
            head_dim=cfg["head_dim"],
            value_head_dim=cfg.get("value_head_dim", None),
            dtype=cfg["dtype"],
            is_sliding_window=use_sliding_window,
        )

        self.norm1 = PytorchRMSNorm(cfg["emb_dim"], dtype=cfg["dtype"])
        self.norm2 = PytorchRMSNorm(cfg["emb_dim"], dtype=cfg["dtype"])

        if use_moe:
            self.feed_forward = DeepSeekMoE(cfg)
        else:
            self.feed_forward = FFN(cfg)

    def forward(self, x, mask, cos, sin, attn_mask=None, _runtime=None):
        ops_mimo.refuse_attn_mask(attn_mask, "TransformerBlock")
        B, S, _ = x.shape
        rt = _runtime if _runtime is not None else ops_mimo.make_runtime(self, B, S, self.window_size, cos, sin, self.context_length)
        return ops_mimo.run_block(self, x, rt)
