"""MiMo-V2-Flash with Multi-Token-Prediction modules on HIP kernels -- API of ``llm_quest/xiaomi/mimo_v2_flash_model.py`` (MTPModule, MainModel,
MiMoModel), bf16 training path and no-grad forward.

Extensions over the reference signatures: ``MainModel.forward_hidden`` (final-normed hidden states and the last block's output, the head not yet
applied: the loss runs the head and the cross entropy as one node), ``MTPModule.forward_hidden`` likewise, and ``MiMoModel.arenas()``.
"""

import torch
import torch.nn as nn

from llm_quest_amd import _lib as L
from llm_quest_amd import ops, ops_dsmoe, ops_g3, ops_mimo
from llm_quest_amd.arena import ParamArena
from llm_quest_amd.common.buffers import GlobalBuffers
from llm_quest_amd.llama3_to_deepseekv3.deepseek_model import _head_loss, _OutLayer
from llm_quest_amd.qwen.qwen3.qwen3_attention import PytorchRMSNorm
from llm_quest_amd.qwen.qwen3.qwen3_model import _Embedding
from llm_quest_amd.xiaomi.mimo_v2_flash_transformer_block import TransformerBlock


class _Linear(nn.Linear):
    """nn.Linear(bias=False) whose forward is the NT GEMM and whose weight gradient goes to the owner's arena."""

    def forward(self, x):
        L.require_gpu(x)
        ops_g3.check_bf16(self, "Linear")
        return ops.LinearFn.apply(x, self, self.weight, None, False)


class MTPModule(nn.Module):
    """One Multi-Token-Prediction module (mimo_v2_flash_model.py:10-49): the embeddings of the shifted tokens and the previous hidden states, each
    RMS-normed, concatenated and projected down to emb_dim, then one sliding-window block with a dense FFN, a final norm and the shared head."""

    def __init__(self, cfg, main_output_head):
        super().__init__()
        self.out_layer = main_output_head  # shared

        self.rms_h_prev = PytorchRMSNorm(cfg["emb_dim"], dtype=cfg["dtype"])
        self.rms_input = PytorchRMSNorm(cfg["emb_dim"], dtype=cfg["dtype"])
        self.final_norm = PytorchRMSNorm(cfg["emb_dim"], dtype=cfg["dtype"])

        self.down_proj = _Linear(2 * cfg["emb_dim"], cfg["emb_dim"], bias=False, dtype=cfg["dtype"])

        self.trf_block = TransformerBlock(cfg, layer_idx=0, use_sliding_window=True, use_moe=False)

    def _build_arena(self):
        if getattr(self, "_own_arena", None) is None:
            named = [(n, p) for n, p in self.named_parameters() if not n.startswith("out_layer.")]
            ar = ParamArena(named)
            for m in (self.rms_h_prev, self.rms_input, self.final_norm, self.down_proj, *self.trf_block.modules()):
                object.__setattr__(m, "_arena", ar)
            object.__setattr__(self, "_own_arena", ar)
        return self._own_arena

    def forward_hidden(self, x_embeds, h_prev, mask, cos, sin):
        """-> (final-normed hidden states, h_curr): what ``forward`` applies the head to, and the block output."""
        self._build_arena()
        x = self.rms_input(x_embeds)
        h_prev = self.rms_h_prev(h_prev)
        x = self.down_proj(torch.cat([x, h_prev], dim=-1))
        h_curr = self.trf_block(x, mask, cos, sin)
        return self.final_norm(h_curr), h_curr

    def forward(self, x_embeds, h_prev, mask, cos, sin):
        hidden, h_curr = self.forward_hidden(x_embeds, h_prev, mask, cos, sin)
        return self.out_layer(hidden), h_curr


class MainModel(nn.Module):
    """Embedding, the blocks, final norm and head; returns (logits, h_final) (mimo_v2_flash_model.py:52-124).  Layer 0 is global attention with a
    dense FFN; layers i >= 1 hold a DeepSeekMoE and use sliding-window attention unless (i + 1) % hybrid_ratio == 0.  Two RoPE table sets (``rope_base``
    for the windowed layers, ``rope_base_ga`` for the global ones, both with ``partial_rope_factor``) and both mask buffers are registered as
    upstream; the kernels never read the masks."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg

        self.emb_layer = _Embedding(num_embeddings=cfg["vocab_size"], embedding_dim=cfg["emb_dim"], dtype=cfg["dtype"])

        self.layers = nn.ModuleList()
        for i in range(cfg["n_layers"]):
            if i == 0:
                use_swa = False
                use_moe = False
            else:
                use_moe = True
                use_swa = True if (i + 1) % cfg["hybrid_ratio"] else False

            self.layers.append(TransformerBlock(cfg, layer_idx=i, use_sliding_window=use_swa, use_moe=use_moe))

        self.final_norm = PytorchRMSNorm(cfg["emb_dim"], dtype=cfg["dtype"])
        self.out_head = _OutLayer(cfg["emb_dim"], cfg["vocab_size"], bias=False, dtype=cfg["dtype"])

        self.rope_base_swa = cfg.get("rope_base", 10000)
        self.rope_base_ga = cfg.get("rope_base_ga", 640000)

        mask_swa = GlobalBuffers.get_swa_mask(cfg["context_length"], cfg["window_size"])
        cos_swa, sin_swa = GlobalBuffers.get_rope_params(
            ctx_len=cfg["context_length"],
            rope_base=self.rope_base_swa,
            head_dim=cfg["head_dim"],
            rotation_factor=cfg["partial_rope_factor"],
        )
        self.register_buffer("mask_swa", mask_swa)
        self.register_buffer("cos_swa", cos_swa)
        self.register_buffer("sin_swa", sin_swa)

        mask_ga = GlobalBuffers.get_causal_mask(cfg["context_length"])
        cos_ga, sin_ga = GlobalBuffers.get_rope_params(
            ctx_len=cfg["context_length"],
            rope_base=self.rope_base_ga,
            head_dim=cfg["head_dim"],
            rotation_factor=cfg["partial_rope_factor"],
        )
        self.register_buffer("mask_ga", mask_ga)
        self.register_buffer("cos_ga", cos_ga)
        self.register_buffer("sin_ga", sin_ga)
        self._arenas_built = False

    def _build_arenas(self):
        if self._arenas_built:
            return
        for blk in self.layers:
            ar = ParamArena(ops_dsmoe.arena_named_params(blk))  # a routed expert's lin_gate in front of its lin1; the dense block unchanged
            for m in blk.modules():
                object.__setattr__(m, "_arena", ar)
        ar = ParamArena([("emb_layer.weight", self.emb_layer.weight), ("final_norm.weight", self.final_norm.weight), ("out_head.weight", self.out_head.weight)])
        for m in (self.emb_layer, self.final_norm, self.out_head):
            object.__setattr__(m, "_arena", ar)
        object.__setattr__(self, "_top_arena", ar)
        self._arenas_built = True

    def forward_hidden(self, x, attn_mask=None):
        """(b, s) ids -> (final-normed hidden states, h_final), both (b, s, emb)."""
        L.require_gpu(x)
        ops_g3.check_bf16(self, "MainModel")
        ops_mimo.refuse_attn_mask(attn_mask, "MainModel")
        self._build_arenas()
        B, S = x.shape
        ctx = self.cfg["context_length"]
        rt = {True: ops_mimo.make_runtime(self, B, S, self.cfg["window_size"], self.cos_swa, self.sin_swa, ctx),
              False: ops_mimo.make_runtime(self, B, S, None, self.cos_ga, self.sin_ga, ctx)}
        x = self.emb_layer(x)

        for layer in self.layers:
            if layer.use_sliding_window:
                mask, cos, sin = self.mask_swa, self.cos_swa, self.sin_swa
            else:
                mask, cos, sin = self.mask_ga, self.cos_ga, self.sin_ga

            x = layer(x, mask, cos, sin, attn_mask, _runtime=rt[layer.use_sliding_window])

        h_final = x
        return self.final_norm(x), h_final

    def forward(self, x, attn_mask=None):
        x, h_final = self.forward_hidden(x, attn_mask)
        logits = self.out_head(x)
        return logits, h_final


class MiMoModel(nn.Module):
    """Main model + ``mtp_depth`` MTP modules sharing its embedding and head (mimo_v2_flash_model.py:130-210).

    ``forward(x, targets)``: eval mode without targets returns the main logits; eval mode or ``mtp_depth == 0`` the main loss; training the total
    loss ``main + mtp_loss_coeff / mtp_depth * sum_k CE(mtp_k)``, where MTP step k runs on the sliced sequence of length s - k - 1 with the
    sliding-window tables from position 0 and is scored against the input ids shifted by k + 1, as upstream.  Every CE ignores -100 and runs fused
    with the head; the loss is returned in the logits' dtype (bf16), as ``F.cross_entropy`` on bf16 logits does."""

    def __init__(self, cfg):
        super().__init__()
        self.main_model = MainModel(cfg)
        self.mtp_depth = cfg.get("mtp_depth", 0)
        self.mtp_coeff = cfg.get("mtp_loss_coeff", 0.0)

        self.mtp_modules = nn.ModuleList([MTPModule(cfg, self.main_model.out_head) for _ in range(self.mtp_depth)])

    def arenas(self):
        """Gradient buckets in backward-completion order: MTP modules last -> first, main blocks last -> first, then the shared top arena."""
        self.main_model._build_arenas()
        return ([m._build_arena() for m in reversed(self.mtp_modules)] + [blk._arena for blk in reversed(self.main_model.layers)]
                + [self.main_model._top_arena])

    def forward(self, x, targets=None):
        L.require_gpu(x)
        ops_g3.check_bf16(self, "MiMoModel")
        main = self.main_model
        hidden, h_prev = main.forward_hidden(x)
        dtype = main.out_head.weight.dtype

        if not self.training and targets is None:
            return main.out_head(hidden)

        if targets is None:
            raise ValueError("targets must be provided when computing loss")

        main_loss = _head_loss(main.out_head, hidden, targets)

        if not self.training or self.mtp_depth == 0:
            return main_loss.to(dtype)

        mtp_mask = main.mask_swa
        mtp_cos = main.cos_swa
        mtp_sin = main.sin_swa

        x_embeds = main.emb_layer(x)

        mtp_loss_total = 0
        for i, mtp_module in enumerate(self.mtp_modules):
            k = i + 1
            mtp_slice = x_embeds[:, k:-1]
            mtp_target = x[:, k + 1 :]

            if k == 1:
                h_slice = h_prev[:, :-2]
            else:
                h_slice = h_prev[:, :-1]

            seq_len = h_slice.shape[1]
            if seq_len == 0:
                break
            curr_cos = mtp_cos[:seq_len]
            curr_sin = mtp_sin[:seq_len]

            mtp_hidden, h_curr = mtp_module.forward_hidden(mtp_slice, h_slice, mtp_mask, curr_cos, curr_sin)

            mtp_loss_total = mtp_loss_total + _head_loss(mtp_module.out_layer, mtp_hidden, mtp_target)

            h_prev = h_curr

        total_loss = main_loss + (self.mtp_coeff / self.mtp_depth) * mtp_loss_total

        return total_loss.to(dtype)
