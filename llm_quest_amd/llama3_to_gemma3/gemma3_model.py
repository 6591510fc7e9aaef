"""Gemma3 on HIP kernels -- API of ``llm_quest/llama3_to_gemma3/gemma3_model.py`` (Gemma3Model), bf16 training path.

Extensions over the reference signature, as on ``Qwen3Model``: ``forward_hidden`` / ``lm_loss`` (the engine's fast path: final-normed hidden
states, then the tied head and the cross entropy in one node) and ``arenas()`` (one gradient bucket per block plus one for the rest).
"""

import torch
import torch.nn as nn

from llm_quest_amd import _lib as L
from llm_quest_amd import ops, ops_g3
from llm_quest_amd.arena import ParamArena
from llm_quest_amd.common.buffers import GlobalBuffers
from llm_quest_amd.llama3_to_gemma3.gemma3_transformer_block import RMSNorm, TransformerBlock
from llm_quest_amd.qwen.qwen3.qwen3_model import _Embedding, _OutHead


class Gemma3Model(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.emb_dict = _Embedding(cfg["vocab_size"], cfg["emb_dim"], dtype=cfg["dtype"])
        self.trf_blocks = nn.ModuleList([TransformerBlock(cfg, layer) for layer in range(cfg["n_layers"])])
        self.final_norm = RMSNorm(cfg["emb_dim"])
        self.out_head = _OutHead(self.emb_dict.weight)  # weights tying (gemma3_model.py:51)
        self.context_length = cfg["context_length"]
        cos, sin = GlobalBuffers.get_rope_params(cfg["context_length"], cfg["rope_base"], cfg["emb_dim"] // cfg["n_heads"])
        self.register_buffer("mask", GlobalBuffers.get_causal_mask(cfg["context_length"]))
        self.register_buffer("cos", cos)
        self.register_buffer("sin", sin)
        self.register_buffer("swa_mask", GlobalBuffers.get_swa_buffers(cfg["context_length"], cfg["window_size"]))
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
        """Gradient buckets in backward-completion order: blocks last -> first, then the top arena (tied head + embedding + final norm)."""
        self._build_arenas()
        return [blk._arena for blk in reversed(self.trf_blocks)] + [self._top_arena]

    # ------------------------------------------------------------------ forward paths
    def forward_hidden(self, x, attn_mask=None):
        """Embedding, blocks and final norm: (b, s) ids -> (b, s, emb).  ``attn_mask`` is the ignored ghost argument it is upstream."""
        L.require_gpu(x)
        ops_g3.check_bf16(self, "Gemma3Model")
        self._build_arenas()
        B, S = x.shape
        if S > self.context_length:
            raise ValueError(f"sequence length {S} exceeds context_length {self.context_length}")
        rt = ops_g3.make_runtime(self, B, S, self.cos, self.sin)
        x = self.emb_dict(x)
        for blk in self.trf_blocks:
            x = blk(x, self.mask, self.cos, self.sin, self.swa_mask, _runtime=rt)
        return self.final_norm(x)

    def forward(self, x, attn_mask=None):
        """Logits (b, s, vocab) in the model dtype (reference: gemma3_model.py:54-64)."""
        return self.out_head(self.forward_hidden(x, attn_mask))

    def lm_loss(self, hidden_rows, targets):
        """Mean CE (ignore_index=-100) of the tied head on ``hidden_rows`` (rows, emb) vs ``targets`` (rows,)."""
        self._build_arenas()
        h = hidden_rows if hidden_rows.is_contiguous() else hidden_rows.contiguous()
        t = targets.reshape(-1).contiguous()
        return ops.LMHeadLossFn.apply(h, t, self.out_head, self.out_head.weight, torch.is_grad_enabled())
