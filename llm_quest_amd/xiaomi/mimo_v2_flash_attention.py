"""Grouped-query attention with an attention sink -- API of ``llm_quest/xiaomi/mimo_v2_flash_attention.py`` (bf16 training path, no-grad forward).

The reference builds the dense score matrix, masks it, appends one sink column per head for the softmax and slices it off again; here the core is
``mi355_sink_attn_fwd/_bwd`` (csrc/attention_band.hip): the band is computed from indices, the sink is merged into the online softmax's state once behind the key loop (one more key without a value), the v / o
heads have their own width, and ``mask`` is never read inside the model (``TransformerBlock`` hands the window over as a number).  Called on its
own, the module has only the mask to learn the window from: it is read once per mask on the host (``ops_mimo.window_of``) and must be the causal mask
or a sliding-window band.
"""

import torch
import torch.nn as nn

from llm_quest_amd import kernels_mimo as KM
from llm_quest_amd import ops_mimo
from llm_quest_amd.qwen.qwen3.qwen3_attention import PytorchRMSNorm


class GroupedQueryAttentionWithSink(nn.Module):
    """GQA with QK-RMSNorm before a partial RoPE, value heads of their own width and, on sliding-window layers, one learnable sink logit per
    query head that enters the softmax denominator only (mimo_v2_flash_attention.py:16-132).  (head_dim, value_head_dim) must be a built pair
    (``kernels_mimo.HEAD_DIM_PAIRS``); any ``num_heads / num_kv_groups`` ratio works."""

    def __init__(
        self,
        d_in,
        num_heads,
        num_kv_groups,
        head_dim,
        value_head_dim=None,
        dtype=None,
        is_sliding_window=False,
    ):
        super().__init__()
        assert num_heads % num_kv_groups == 0, "num_heads must be divisible by num_kv_groups"

        self.num_heads = num_heads
        self.head_dim = head_dim
        self.value_head_dim = value_head_dim if value_head_dim is not None else head_dim
        KM.check_pair(self.head_dim, self.value_head_dim, "GroupedQueryAttentionWithSink")
        self.d_out = num_heads * self.value_head_dim
        self.num_kv_groups = num_kv_groups
        self.num_repeat = num_heads // num_kv_groups
        self.att_scaling = head_dim**-0.5
        self.is_sliding_window = is_sliding_window

        # declaration order = arena order: q | k | v must be adjacent for the fused projection
        self.w_queries = nn.Linear(d_in, num_heads * head_dim, bias=False, dtype=dtype)
        self.w_keys = nn.Linear(d_in, num_kv_groups * head_dim, bias=False, dtype=dtype)
        self.w_values = nn.Linear(d_in, num_kv_groups * self.value_head_dim, bias=False, dtype=dtype)
        self.out_proj = nn.Linear(self.d_out, d_in, bias=False, dtype=dtype)

        self.q_norm = PytorchRMSNorm(head_dim, dtype=dtype)
        self.k_norm = PytorchRMSNorm(head_dim, dtype=dtype)

        if is_sliding_window:
            self.sink = nn.Parameter(torch.normal(mean=0.0, std=0.02, size=(num_heads,), dtype=dtype))

    def forward(self, x, mask, cos, sin, attn_mask=None, _runtime=None):
        """x (b, s, d_in); cos / sin (>= s, R) with R the rotated width; ``mask`` gives the window when the module is called on its own."""
        ops_mimo._check_activation(x, "GroupedQueryAttentionWithSink")
        ops_mimo.refuse_attn_mask(attn_mask, "GroupedQueryAttentionWithSink")
        B, S, _ = x.shape
        rt = _runtime
        if rt is None:
            W = ops_mimo.window_of(mask, S) if S > 0 else 1
            rt = ops_mimo.make_runtime(self, B, S, W, cos, sin)
        return ops_mimo.run_attention(self, x, rt)
