"""Gemma3 attention -- API of ``llm_quest/llama3_to_gemma3/gemma3_attention.py``: LayerNorm (the QK norm), sliding-window attention and
GroupedQueryAttention with the local / global layer schedule.

The reference materialises a [b, h, s, w, d] gather of key / value windows; here a windowed layer runs ``mi355_swa_attn_fwd/_bwd``
(csrc/attention_band.hip), which walks only the key tiles inside the band and never reads ``swa_mask`` or ``mask``.
"""

import torch
import torch.nn as nn

from llm_quest_amd import _lib as L
from llm_quest_amd import ops_g3


class LayerNorm(nn.Module):
    """scale * (x - mean) / (std + eps) + shift over the last dim, population std (gemma3_attention.py:13-43).

    The module exists upstream as the QK norm over head_dim; called on its own it runs the RoPE + LayerNorm kernel with an identity rotation,
    so ``emb_dim`` must be one of the head dims that kernel is built for (32, 64, 128) -- upstream takes any width; another one raises ValueError."""

    def __init__(self, emb_dim):
        super().__init__()
        self.eps = 1e-5
        self.scale = nn.Parameter(torch.ones(emb_dim))
        self.shift = nn.Parameter(torch.zeros(emb_dim))

    def forward(self, x):
        ops_g3._check_activation(x, "LayerNorm")
        ops_g3.check_bf16(self, "LayerNorm")
        return ops_g3.LayerNormFn.apply(x, self, self.scale, self.shift)


def apply_sliding_window_attention(queries, keys, values, window_size, swa_mask=None):
    """(b, heads, s, head_dim) queries / keys / values -> context (b, heads, s, head_dim): query i attends to keys i - window_size < j <= i.
    ``swa_mask`` is accepted for signature compatibility and never read: the band is computed from indices."""
    for t in (queries, keys, values):
        ops_g3._check_activation(t, "apply_sliding_window_attention")
    if queries.dim() != 4 or keys.shape != values.shape or keys.shape[0] != queries.shape[0] or keys.shape[2:] != queries.shape[2:]:
        raise ValueError(f"apply_sliding_window_attention: expected (b, heads, s, head_dim) tensors, got {tuple(queries.shape)}, {tuple(keys.shape)}, {tuple(values.shape)}")
    return ops_g3.SlidingWindowFn.apply(queries, keys, values, int(window_size))


class GroupedQueryAttention(nn.Module):
    """GQA with RoPE, per-head LayerNorm of q and k, and sliding-window attention on the layers the schedule makes local
    (gemma3_attention.py:131-242): a layer is windowed when window_size > 0 and (layer_id + 1) % (local_global_att_ratio + 1) != 0."""

    def __init__(self, d_in, d_out, num_heads, num_kv_groups, window_size, layer_id, dtype=None, local_global_att_ratio=5):
        super().__init__()
        assert d_out % num_heads == 0, "d_out must be divisible by num_heads"
        assert num_heads % num_kv_groups == 0, "num_heads must be divisible by num_kv_groups"
        self.num_heads = num_heads
        self.d_out = d_out
        self.head_dim = d_out // num_heads
        self.num_kv_groups = num_kv_groups
        self.num_repeat = num_heads // num_kv_groups
        self.att_scaling = self.head_dim**-0.5
        # w_queries | w_keys | w_values: adjacent in the arena -> one QKV GEMM
        self.w_queries = nn.Linear(d_in, d_out, bias=False, dtype=dtype)
        self.w_keys = nn.Linear(d_in, num_kv_groups * self.head_dim, bias=False, dtype=dtype)
        self.w_values = nn.Linear(d_in, num_kv_groups * self.head_dim, bias=False, dtype=dtype)
        self.out_proj = nn.Linear(d_out, d_out, dtype=dtype)
        self.window_size = window_size
        self.layer_id = layer_id
        self.lg_ratio = local_global_att_ratio + 1
        self.q_norm = LayerNorm(self.head_dim)
        self.k_norm = LayerNorm(self.head_dim)

    @property
    def is_windowed(self):
        return self.window_size > 0 and (self.layer_id + 1) % self.lg_ratio != 0

    def forward(self, x, mask, cos, sin, swa_mask=None, _runtime=None):
        ops_g3._check_activation(x, "GroupedQueryAttention")
        ops_g3.check_bf16(self, "GroupedQueryAttention")
        B, S, _ = x.shape
        rt = _runtime if _runtime is not None else ops_g3.make_runtime(self, B, S, cos, sin)
        return ops_g3.AttentionFn.apply(x, self, rt, torch.is_grad_enabled(), *ops_g3._param_list(self))
