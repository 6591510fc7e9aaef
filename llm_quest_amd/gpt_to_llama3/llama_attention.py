"""Grouped-query attention with RoPE -- API of ``llm_quest/gpt_to_llama3/llama_attention.py``.

The reference rotates transposed (b, heads, s, head_dim) tensors, repeats the key / value heads and runs a dense masked softmax; here the heads
never move: one NT GEMM on the fused ``[w_queries | w_keys | w_values]``, ``mi355_llama_rope_fwd`` on the packed result, the tuned causal
``mi355_attn_fwd`` with the key mask, and the out-projection with its bias on the GEMM epilogue.  ``mask`` is never read (causality is computed
from indices).  There is no QK-norm in this family, so its attention logits are unbounded: ``track_max_attn_logit`` makes every forward leave the
per-head maximum in ``max_attn_logit`` for ``common/qk_clip.py``.
"""

import torch.nn as nn

from llm_quest_amd import ops_g3, ops_llama


class GroupedQueryAttention(nn.Module):
    """``num_kv_groups`` key / value heads shared by groups of ``num_heads / num_kv_groups`` query heads (llama_attention.py:14-110).  head_dim
    must be 64 or 128.

    ``track_max_attn_logit`` (a plain attribute, default False): when True every forward, in grad mode or not, also launches
    ``mi355_attn_max_logit`` on the post-RoPE q and k and stores the result in ``max_attn_logit`` (fp32 [num_heads] on the device, overwritten per
    forward).  When False the forward launches nothing more than it would without the feature.

    ``expose_qk`` (a plain attribute, default False; ours): when True and grad mode is on, the autograd node of the forward (the block's, or this
    module's when called on its own) returns the post-RoPE q [b * s, num_heads * head_dim] and k [b * s, num_kv_groups * head_dim] as two more
    differentiable outputs and leaves them in ``exposed_qk`` (``common/reinforced_attention_learning.py`` reads them); gradients that arrive on them
    join dq, dk ahead of the RoPE backward.  When False the node has one output and the forward launches what it launches without the feature."""

    def __init__(
        self,
        d_in,
        d_out,
        num_heads,
        num_kv_groups,
        dtype=None,
    ):
        super().__init__()
        if d_out % num_heads != 0:
            raise ValueError("d_out must be divisible by num_heads")
        if num_heads % num_kv_groups != 0:
            raise ValueError("num_heads must be divisible by num_kv_groups")

        self.num_heads = num_heads
        self.d_out = d_out
        self.head_dim = d_out // self.num_heads
        ops_llama.check_head_dim(self.head_dim)
        self.att_scaling = self.head_dim**-0.5
        self.num_kv_groups = num_kv_groups
        self.num_repeat = self.num_heads // self.num_kv_groups
        # w_queries, w_keys, w_values: adjacent in the arena -> one [(Hq + 2 Hkv) * D, d_in] GEMM
        self.w_queries = nn.Linear(d_in, d_out, bias=False, dtype=dtype)
        self.w_keys = nn.Linear(d_in, num_kv_groups * self.head_dim, bias=False, dtype=dtype)
        self.w_values = nn.Linear(d_in, num_kv_groups * self.head_dim, bias=False, dtype=dtype)
        self.out_proj = nn.Linear(d_out, d_out, dtype=dtype)
        self.track_max_attn_logit = False
        self.max_attn_logit = None
        self.expose_qk = False
        self.exposed_qk = None

    def forward(self, x, mask, cos, sin, attn_mask=None, _runtime=None):
        ops_g3._check_activation(x, "GroupedQueryAttention")
        ops_llama.check_bf16(self, "GroupedQueryAttention")
        B, S, _ = x.shape
        rt = _runtime if _runtime is not None else ops_llama.make_runtime(self, B, S, cos, sin, attn_mask)
        return ops_llama.run_attention(self, x, rt)
