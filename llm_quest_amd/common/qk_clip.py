"""QK-Clip (MuonClip's rescaling of the query / key weights whose attention logits grew past a threshold) -- API of ``llm_quest/common/qk_clip.py``
(QKClipNaive, QKClip, MagnitudeQKClipMHA), applied after the optimizer step.

Upstream reads the per-head maxima off the materialised (b, heads, s, s) scores and decides on the host (``.any()``) which layers to touch.  Here
the maxima come from ``mi355_attn_max_logit`` (``GroupedQueryAttention.track_max_attn_logit``; ``collect_max_attn_logits`` gathers them) and each
layer is ONE ``mi355_qk_clip`` launch on that layer's ``att.w_queries.weight`` / ``att.w_keys.weight`` -- views of the block's parameter arena --
which computes gamma on the device and writes only the heads that clip.  Nothing is read back to the host.

One deviation: a maximum that is NaN, infinite or not positive never clips.  Upstream's ``QKClipNaive`` computes ``clamp(tau / m, max=1)``, which is
negative for ``m < 0`` and turns the weights into NaN through the fractional power.
"""

import torch

from llm_quest_amd import kernels_llama as KL


def collect_max_attn_logits(model):
    """The per-layer list ``QKClip`` takes: ``att.max_attn_logit`` (fp32 [num_heads], device) of every block, as the last tracked forward left them."""
    out = []
    for i, blk in enumerate(model.trf_blocks):
        m = getattr(blk.att, "max_attn_logit", None)
        if m is None:
            raise RuntimeError(f"trf_blocks[{i}].att holds no max_attn_logit: set att.track_max_attn_logit = True before the forward")
        out.append(m)
    return out


class _QKClipBase:
    _mode = None

    def __init__(self, clip_threshold, alpha=0.5):
        self.clip_threshold = clip_threshold
        self.alpha = alpha
        self.cached_qk_layers = None  # references to the parameters (their .data are arena views and may be rebuilt: read per call)
        self.num_query_heads = None
        self.num_kv_heads = None
        self.head_dim = None

    def _init_cache(self, model):
        if self.cached_qk_layers is None:
            self.cached_qk_layers = [(blk.att.w_queries.weight, blk.att.w_keys.weight) for blk in model.trf_blocks]
            att = model.trf_blocks[0].att
            self.num_query_heads = att.num_heads
            self.num_kv_heads = getattr(att, "num_kv_groups", self.num_query_heads)
            self.head_dim = att.w_queries.weight.shape[0] // self.num_query_heads

    @torch.no_grad()
    def _apply(self, model, max_attn_logits_per_layer):
        """``max_attn_logits_per_layer``: a list with one fp32 [num_heads] device tensor per layer.  Modifies the weights in place."""
        self._init_cache(model)
        if len(max_attn_logits_per_layer) > len(self.cached_qk_layers):
            raise ValueError(f"{type(self).__name__}: {len(max_attn_logits_per_layer)} layers of maxima for a model of {len(self.cached_qk_layers)} layers")
        if self._mode == "magnitude" and self.num_query_heads != self.num_kv_heads:
            raise ValueError("MagnitudeQKClipMHA is defined for multi-head attention only (num_heads == num_kv_groups)")
        for (wq, wk), m in zip(self.cached_qk_layers, max_attn_logits_per_layer):
            if self._mode == "naive" and m.numel() == 1:  # upstream's naive class takes one maximum per layer
                m = m.reshape(1).expand(self.num_query_heads).contiguous()
            KL.qk_clip_(wq.data, wk.data, m, self.num_query_heads, self.num_kv_heads, self.clip_threshold, self.alpha, self._mode)


class QKClipNaive(_QKClipBase):
    """One gamma per layer from its largest head; every row of W_q and W_k of a layer that clips is scaled by gamma^alpha resp. gamma^(1 - alpha)
    (qk_clip.py:23-77).  Takes the same per-head maxima as ``QKClip``; the layer maximum is taken on the device."""

    _mode = "naive"

    def __init__(self, clip_threshold, alpha=0.5):
        super().__init__(clip_threshold, alpha)

    def __call__(self, model, max_attention_logits):
        self._apply(model, max_attention_logits)


class QKClip(_QKClipBase):
    """Per head: query head h clips iff m_h > tau, gamma_h = tau / m_h, its rows of W_q are scaled by gamma_h^alpha; a key head takes the minimum
    gamma of its query heads and is scaled by gamma^(1 - alpha) (qk_clip.py:80-203).  MHA, GQA and MQA."""

    _mode = "per_head"

    def __init__(self, clip_threshold, alpha=0.5):
        super().__init__(clip_threshold, alpha)

    def __call__(self, model, max_attn_logits_per_layer):
        self._apply(model, max_attn_logits_per_layer)


class MagnitudeQKClipMHA(_QKClipBase):
    """Per head on the magnitude: gamma_h = min(1, tau / |m_h|) (qk_clip.py:209-271).  Multi-head attention only: ``ValueError`` on a GQA model."""

    _mode = "magnitude"

    def __init__(self, clip_threshold, alpha=0.5):
        super().__init__(clip_threshold, alpha)

    def __call__(self, model, max_attn_logits_per_layer):
        self._apply(model, max_attn_logits_per_layer)
