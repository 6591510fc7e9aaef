"""Multi-head Latent Attention -- API of ``llm_quest/llama3_to_deepseekv3/deepseek_attention.py`` (training form, no latent cache).

The reference concatenates ``[q_nope | q_rope]`` and ``[k_nope | expand(k_rope)]`` per head and runs a dense masked softmax; here the
attention core is ``mi355_mla_attn_fwd/_bwd`` (csrc/deepseek.hip), which reads the two halves of the score contraction from their own
tensors and the decoupled key once per token, and never reads ``mask``.
"""

import torch
import torch.nn as nn

from llm_quest_amd import ops_g3, ops_mla


class RMSNorm(nn.Module):
    """scale * x / (RMS(x) + eps): eps is added to the RMS (the reference imports it from gpt_to_llama3/llama_transformer_block.py:15-38)."""

    def __init__(self, emb_dim, dtype=None):
        super().__init__()
        self.eps = 1e-6
        self.scale = nn.Parameter(torch.ones(emb_dim, dtype=dtype))

    def forward(self, x):
        ops_g3._check_activation(x, "RMSNorm")
        ops_g3.check_bf16(self, "RMSNorm")
        return ops_g3.RMSNormFn.apply(x, self, self.scale)


class MultiLatentAttention(nn.Module):
    """Low-rank query and key / value latents with their own RMSNorms, per-head up projections, and a decoupled rotary part: ``head_dim / 2``
    extra features per query head and ONE ``head_dim / 2``-wide key per token shared by all heads (deepseek_attention.py:9-110).
    ``q_rank`` = 1536 and ``kv_rank`` = 4 * head_dim are hard-coded upstream and stay so.  head_dim must be 64 or 128."""

    def __init__(
        self,
        d_in,
        d_out,
        num_heads,
    ):
        super().__init__()
        if d_out % num_heads != 0:
            raise ValueError("d_out must be divisible by num_heads")

        self.d_out = d_out
        self.num_heads = num_heads
        self.head_dim = d_out // self.num_heads
        ops_mla.check_head_dim(self.head_dim)
        self.q_rank = 1536
        self.kv_rank = 4 * self.head_dim
        self.decoup_head_dim = self.head_dim // 2
        self.att_scaling = (self.head_dim + self.decoup_head_dim) ** -0.5
        self.out_proj = nn.Linear(d_out, d_out)

        self.wq_down_proj = nn.Linear(d_in, self.q_rank)
        self.wq_up_proj = nn.Linear(self.q_rank, d_out)
        self.wq_decoup = nn.Linear(self.q_rank, num_heads * self.decoup_head_dim)
        self.wkv_down_proj = nn.Linear(d_in, self.kv_rank)
        self.wk_up_proj = nn.Linear(self.kv_rank, d_out)
        self.wv_up_proj = nn.Linear(self.kv_rank, d_out)
        self.wk_decoup = nn.Linear(d_in, self.decoup_head_dim)

        self.q_rms_norm = RMSNorm(emb_dim=self.q_rank)
        self.kv_rms_norm = RMSNorm(emb_dim=self.kv_rank)

    def forward(self, x, mask, cos, sin, _runtime=None):
        ops_g3._check_activation(x, "MultiLatentAttention")
        ops_g3.check_bf16(self, "MultiLatentAttention")
        B, S, _ = x.shape
        ops_mla.check_mask(mask, S)
        rt = _runtime if _runtime is not None else ops_mla.make_runtime(self, B, S, cos, sin)
        return ops_mla.MLAFn.apply(x, self, rt, torch.is_grad_enabled(), *ops_mla._param_list(self))
