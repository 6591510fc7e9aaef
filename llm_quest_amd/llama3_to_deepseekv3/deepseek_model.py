"""DeepSeek-V3 model with Multi-Token-Prediction modules on HIP kernels -- API of
``llm_quest/llama3_to_deepseekv3/deepseek_model.py`` (MTPModule, MainModel, DeepSeekV3Model), bf16 training path.

Blocks ``layer < cfg["num_ffn"]`` are dense, the rest hold a ``DeepSeekMoE`` (their config keys are checked there); the MTP blocks are dense.
Extensions over the reference signatures: ``MainModel.forward_hidden`` (final-normed hidden states and the block output, the head not yet
applied: the loss runs the head and the cross entropy as one node) and ``DeepSeekV3Model.arenas()``.
"""

import torch
import torch.nn as nn

from llm_quest_amd import _lib as L
from llm_quest_amd import ops, ops_dsmoe, ops_mla
from llm_quest_amd.arena import ParamArena
from llm_quest_amd.common.buffers import GlobalBuffers
from llm_quest_amd.llama3_to_deepseekv3.deepseek_transformer_block import RMSNorm, TransformerBlock
from llm_quest_amd.qwen.qwen3.qwen3_model import _Embedding


class _OutLayer(nn.Linear):
    """nn.Linear(emb_dim, vocab_size, bias=False) whose forward is the NT GEMM."""

    def forward(self, x):
        L.require_gpu(x)
        return ops.LinearFn.apply(x, self, self.weight, None, False)


class _BiasLinear(nn.Linear):
    """nn.Linear with a bias whose forward / backward are the GEMMs and a deterministic bias reduction."""

    def forward(self, x):
        L.require_gpu(x)
        ops_mla.check_bf16(self, "Linear")
        return ops_mla.BiasLinearFn.apply(x, self, self.weight, self.bias)


def _head_loss(out_layer, hidden, targets):
    """Mean CE (ignore_index = -100, as F.cross_entropy) of ``out_layer`` on hidden (b, s, emb) against targets (b, s); fp32 scalar."""
    h = hidden.reshape(-1, hidden.shape[-1])
    h = h if h.is_contiguous() else h.contiguous()
    t = targets.reshape(-1).contiguous()
    return ops.LMHeadLossFn.apply(h, t, out_layer, out_layer.weight, torch.is_grad_enabled())


class MTPModule(nn.Module):
    """One Multi-Token-Prediction module (deepseek_model.py:12-49): the shared embedding of the shifted tokens and the previous hidden states,
    each RMS-normed, concatenated and projected down to emb_dim, then one dense transformer block.

    As upstream, the logits are the shared head applied to the DOWN-PROJECTED INPUT ``x``, not to the block output ``h_curr`` (which only
    feeds the next module); reproduced, see DESIGN.md section 4."""

    def __init__(self, cfg, main_emb_layer, main_output_head):
        super().__init__()

        self.emb_layer = main_emb_layer  # shared
        self.rms_h_prev = RMSNorm(cfg["emb_dim"])
        self.rms_input = RMSNorm(cfg["emb_dim"])
        self.down_proj = _BiasLinear(2 * cfg["emb_dim"], cfg["emb_dim"])
        self.trf_block = TransformerBlock(cfg, layer=0)
        self.out_layer = main_output_head  # shared

    def _build_arena(self):
        if getattr(self, "_own_arena", None) is None:
            named = [(n, p) for n, p in self.named_parameters() if not n.startswith(("emb_layer.", "out_layer."))]
            ar = ParamArena(named)
            for m in (self.rms_h_prev, self.rms_input, self.down_proj, *self.trf_block.modules()):
                object.__setattr__(m, "_arena", ar)
            object.__setattr__(self, "_own_arena", ar)
        return self._own_arena

    def forward_parts(self, x, h_prev, mask, cos, sin, _runtime=None):
        """-> (x after down_proj, h_curr): what ``forward`` applies the head to, and the block output."""
        self._build_arena()
        x = self.emb_layer(x)
        x = self.rms_input(x)
        h_prev = self.rms_h_prev(h_prev)
        x = self.down_proj(torch.cat([x, h_prev], dim=-1))
        h_curr = self.trf_block(x, mask, cos, sin, _runtime=_runtime)
        return x, h_curr

    def forward(self, x, h_prev, mask, cos, sin):
        x, h_curr = self.forward_parts(x, h_prev, mask, cos, sin)
        logits = self.out_layer(x)
        return logits, h_curr


class MainModel(nn.Module):
    """Embedding, the blocks, final norm and head; returns (logits, h_curr) with h_curr the last block's output (deepseek_model.py:52-82)."""

    def __init__(self, cfg):
        super().__init__()

        self.emb_layer = _Embedding(
            num_embeddings=cfg["vocab_size"],
            embedding_dim=cfg["emb_dim"],
            dtype=cfg["dtype"],
        )
        self.trf_blocks = nn.ModuleList(
            [TransformerBlock(cfg, layer) for layer in range(cfg["n_layers"])],
        )
        self.final_norm = RMSNorm(cfg["emb_dim"])
        self.out_layer = _OutLayer(cfg["emb_dim"], cfg["vocab_size"], bias=False, dtype=cfg["dtype"])
        self._arenas_built = False

    def _build_arenas(self):
        if self._arenas_built:
            return
        for blk in self.trf_blocks:
            ar = ParamArena(ops_dsmoe.arena_named_params(blk))  # a routed expert's lin_gate in front of its lin1; dense blocks unchanged
            for m in blk.modules():
                object.__setattr__(m, "_arena", ar)
        ar = ParamArena([("emb_layer.weight", self.emb_layer.weight), ("final_norm.scale", self.final_norm.scale), ("out_layer.weight", self.out_layer.weight)])
        for m in (self.emb_layer, self.final_norm, self.out_layer):
            object.__setattr__(m, "_arena", ar)
        object.__setattr__(self, "_top_arena", ar)
        self._arenas_built = True

    def forward_hidden(self, x, mask, cos, sin, _runtime=None):
        """(b, s) ids -> (final-normed hidden states, h_curr), both (b, s, emb)."""
        L.require_gpu(x)
        ops_mla.check_bf16(self, "MainModel")
        self._build_arenas()
        B, S = x.shape
        ops_mla.check_mask(mask, S)
        rt = _runtime if _runtime is not None else ops_mla.make_runtime(self, B, S, cos, sin)
        x = self.emb_layer(x)
        for block in self.trf_blocks:
            x = block(x, mask, cos, sin, _runtime=rt)
        h_curr = x
        return self.final_norm(h_curr), h_curr

    def forward(self, x, mask, cos, sin):
        x, h_curr = self.forward_hidden(x, mask, cos, sin)
        logits = self.out_layer(x)
        return logits, h_curr


class DeepSeekV3Model(nn.Module):
    """Main model + ``mtp_depth`` MTP modules sharing its embedding and head (deepseek_model.py:85-138).

    ``forward(x, y, shifted_x, shifted_y)``: eval mode with ``y is None`` returns the main logits; eval mode or ``mtp_depth == 0`` the main loss;
    training the total loss ``main + mtp_loss_coeff / mtp_depth * sum_k CE(mtp_k)`` (every CE ignores -100).  Losses are fp32 scalars."""

    def __init__(self, cfg):
        super().__init__()
        self.coeff = cfg["mtp_loss_coeff"]
        self.depth = cfg["mtp_depth"]
        self.main_model = MainModel(cfg)
        self.mtp_modules = nn.ModuleList(
            [MTPModule(cfg, self.main_model.emb_layer, self.main_model.out_layer) for _ in range(self.depth)]
        )
        self.context_length = cfg["context_length"]
        mask = GlobalBuffers.get_causal_mask(cfg["context_length"])
        cos, sin = GlobalBuffers.get_rope_params(
            cfg["context_length"],
            cfg["rope_base"],
            cfg["emb_dim"] // cfg["n_heads"] // 2,  # the decoupled q and k: head_dim / 2
        )
        self.register_buffer("mask", mask)
        self.register_buffer("cos", cos)
        self.register_buffer("sin", sin)

    def arenas(self):
        """Gradient buckets in backward-completion order: MTP modules last -> first, main blocks last -> first, then the shared top arena."""
        self.main_model._build_arenas()
        return ([m._build_arena() for m in reversed(self.mtp_modules)] + [blk._arena for blk in reversed(self.main_model.trf_blocks)]
                + [self.main_model._top_arena])

    def forward(self, x, y, shifted_x, shifted_y):
        L.require_gpu(x)
        ops_mla.check_bf16(self, "DeepSeekV3Model")
        B, S = x.shape
        rt = ops_mla.make_runtime(self, B, S, self.cos, self.sin)
        hidden, h_prev = self.main_model.forward_hidden(x, self.mask, self.cos, self.sin, _runtime=rt)

        if not self.training and y is None:
            return self.main_model.out_layer(hidden)

        main_loss = _head_loss(self.main_model.out_layer, hidden, y)

        if not self.training or self.depth == 0:
            return main_loss

        mtp_losses = 0
        for k, mtp_module in enumerate(self.mtp_modules):
            s_x, s_y = shifted_x[k].to(x.device), shifted_y[k].to(x.device)
            x_k, h_curr = mtp_module.forward_parts(s_x, h_prev, self.mask, self.cos, self.sin, _runtime=rt)
            mtp_losses = mtp_losses + _head_loss(mtp_module.out_layer, x_k, s_y)
            h_prev = h_curr

        return main_loss + (self.coeff / self.depth) * mtp_losses
