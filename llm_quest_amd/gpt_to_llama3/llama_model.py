"""Llama 3.2 on HIP kernels -- API of ``llm_quest/gpt_to_llama3/llama_model.py`` (Llama3Model), bf16 training path and no-grad forward.

Extensions over the reference signature: ``arenas()`` (the gradient buckets, as on ``Qwen3Model``: ``ArenaAdamW.attach`` and ``ddp.py`` take it),
``forward_hidden`` / ``lm_loss`` (final-normed hidden states, then the tied head and the cross entropy as one node).
"""

import torch
import torch.nn as nn

from llm_quest_amd import _lib as L
from llm_quest_amd import ops, ops_llama
from llm_quest_amd.arena import ParamArena
from llm_quest_amd.common.buffers import GlobalBuffers
from llm_quest_amd.gpt_to_llama3.llama_transformer_block import RMSNorm, TransformerBlock
from llm_quest_amd.qwen.qwen3.qwen3_model import _Embedding


class _OutHead(nn.Linear):
    """nn.Linear(emb_dim, vocab_size, bias=False) whose forward is the NT GEMM; its weight is the embedding matrix (tied)."""

    def forward(self, x):
        L.require_gpu(x)
        return ops.LinearFn.apply(x, self, self.weight, None, False)


class Llama3Model(nn.Module):
    """Token embedding, the blocks, final RMSNorm and the tied output head (llama_model.py:17-73).  The (ctx, ctx) ``mask`` buffer is produced for
    ``state_dict`` compatibility only: override ``context_length`` of the 1B config (131 072 -> a 17 GB mask) for training runs."""

    def __init__(self, cfg):
        super().__init__()

        self.emb_dict = _Embedding(
            num_embeddings=cfg["vocab_size"],
            embedding_dim=cfg["emb_dim"],
            dtype=cfg["dtype"],
        )
        self.trf_blocks = nn.ModuleList(
            [TransformerBlock(cfg) for layer in range(cfg["n_layers"])],
        )
        self.final_norm = RMSNorm(cfg["emb_dim"])
        self.out_head = _OutHead(cfg["emb_dim"], cfg["vocab_size"], bias=False, dtype=cfg["dtype"])

        mask = GlobalBuffers.get_causal_mask(cfg["context_length"])
        cos, sin = GlobalBuffers.get_rope_params(
            cfg["context_length"],
            cfg["rope_base"],
            cfg["emb_dim"] // cfg["n_heads"],
        )
        self.register_buffer("mask", mask)
        self.register_buffer("cos", cos)
        self.register_buffer("sin", sin)

        if self.emb_dict.weight.shape != self.out_head.weight.shape:
            raise ValueError("Shape mismatch for weight tying")
        self.out_head.weight = self.emb_dict.weight  # weights tying
        self._arenas_built = False

    # ------------------------------------------------------------------ arenas: one per block + one for the rest
    def _build_arenas(self):
        if self._arenas_built:
            return
        for blk in self.trf_blocks:
            ar = ParamArena(list(blk.named_parameters()))
            for m in blk.modules():
                object.__setattr__(m, "_arena", ar)
        ar = ParamArena([("emb_dict.weight", self.emb_dict.weight), ("final_norm.scale", self.final_norm.scale)])
        for m in (self.emb_dict, self.final_norm, self.out_head):
            object.__setattr__(m, "_arena", ar)
        object.__setattr__(self, "_top_arena", ar)
        self._arenas_built = True

    def arenas(self):
        """Gradient buckets in backward-completion order: blocks last -> first, then the top arena (embedding = head, final norm)."""
        self._build_arenas()
        return [blk._arena for blk in reversed(self.trf_blocks)] + [self._top_arena]

    # ------------------------------------------------------------------ forward paths
    def forward_hidden(self, x, attn_mask=None):
        """Blocks + final norm: (b, s) ids -> (b, s, emb)."""
        L.require_gpu(x)
        ops_llama.check_bf16(self, "Llama3Model")
        self._build_arenas()
        B, S = x.shape
        rt = ops_llama.make_runtime(self, B, S, self.cos, self.sin, attn_mask)
        x = self.emb_dict(x)
        for block in self.trf_blocks:
            x = block(x, self.mask, self.cos, self.sin, attn_mask, _runtime=rt)
        return self.final_norm(x)

    def forward(self, x, attn_mask=None):
        """Logits (b, s, vocab), bf16."""
        return self.out_head(self.forward_hidden(x, attn_mask))

    def lm_loss(self, hidden_rows, targets):
        """Mean CE (ignore_index=-100) of the tied head on ``hidden_rows`` (rows, emb) vs ``targets`` (rows,); fp32 scalar."""
        self._build_arenas()
        h = hidden_rows if hidden_rows.is_contiguous() else hidden_rows.contiguous()
        t = targets.reshape(-1).contiguous()
        return ops.LMHeadLossFn.apply(h, t, self.out_head, self.out_head.weight, torch.is_grad_enabled())
