"""Dense Qwen3 with hyper-connections -- API of ``llm_quest/common/hyper_connections/hyper_qwen3.py``.

The residual stream is ``n = expansion_rate`` parallel streams, activations ``[B, S, n, emb]``.  Each half of a block (attention, FFN)
is ONE autograd node:

    forward :  hc_width_fwd (norm of all streams, the three coefficient sets, R = H_res @ x, P = H_pre @ x: one pass over x)
               -> norm1 / norm2 -> attention / FFN, the kernels of the plain Qwen3 block -> hc_depth_fwd (H_post^T y + R)
    backward:  hc_depth_bwd -> the sub-layer's backward -> hc_width_bwd (dx and every coefficient gradient, one pass)

Only classic hyper-connections (``hc_type="hc"``) are implemented, as a training path.
"""

import torch
import torch.nn as nn

from llm_quest_amd import _lib as L
from llm_quest_amd import kernels as K
from llm_quest_amd import kernels_hc as KH
from llm_quest_amd import ops
from llm_quest_amd.arena import ParamArena
from llm_quest_amd.common.hyper_connections.hyper_connections import HyperConnectionPost, HyperConnectionPre, HyperConnectionRes
from llm_quest_amd.qwen.qwen3.qwen3_attention import PytorchRMSNorm
from llm_quest_amd.qwen.qwen3.qwen3_model import Qwen3Model
from llm_quest_amd.qwen.qwen3.qwen3_transformer_block import TransformerBlock

BF16 = torch.bfloat16


def _check_hc_type(hc_type):
    if hc_type in ("mhc", "mhc-lite"):
        raise NotImplementedError(
            f"hc_type={hc_type!r} is not implemented: manifold-constrained hyper-connections need the Sinkhorn-Knopp projection of H_res and the "
            "norm over the flattened n * emb_dim streams, neither of which has a kernel yet; only hc_type='hc' is available"
        )
    if hc_type != "hc":
        raise ValueError(f"Invalid Hyper-Connections type: {hc_type}, must be 'mhc', 'mhc-lite' or 'hc'")


def _create_hyper_connection_set(emb_dim, expansion_rate, dtype):
    """Bundle for classic hyper-connections: norm + res + pre + post for one sub-block (attn or ffn)."""
    return nn.ModuleDict(
        {
            "norm": PytorchRMSNorm(emb_dim, dtype=dtype),
            "res": HyperConnectionRes(emb_dim, expansion_rate=expansion_rate),
            "pre": HyperConnectionPre(emb_dim, expansion_rate=expansion_rate),
            "post": HyperConnectionPost(emb_dim, expansion_rate=expansion_rate),
        }
    )


def _coeffs(hc):
    res, pre, post = hc["res"], hc["pre"], hc["post"]
    return KH.Coeffs(hc["norm"].weight, res.linear.weight, pre.linear.weight, post.linear.weight, res.factor, pre.factor, post.factor,
                     res.bias, pre.bias, post.bias)


def _store_coeff_grads(blk, hc, g):
    """The gradients of one sub-block's connections (fp32 views of the reduced row of partials) into the block's arenas: the 9 coefficient tensors
    live in the fp32 arena, the norm weight in the bf16 one."""
    a32 = blk._hc_arena
    res, pre, post = hc["res"], hc["pre"], hc["post"]
    for p, gv in ((res.factor, g.f_res), (res.bias, g.b_res), (res.linear.weight, g.W_res), (pre.factor, g.f_pre), (pre.bias, g.b_pre),
                  (pre.linear.weight, g.w_pre), (post.factor, g.f_post), (post.bias, g.b_post), (post.linear.weight, g.w_post)):
        if p is None or not p.requires_grad:
            continue
        view, acc = a32.grad_target(p)
        if acc:
            view.add_(gv.view(view.shape))
        else:
            view.copy_(gv.view(view.shape))
    view, acc = ops._vecgrad(blk._arena, hc["norm"].weight)
    if view is not None:
        K.add_f32_to_bf16(g.w_norm, view if acc else None, view)


# ----------------------------------------------------------------------------------------------- the two sub-layers on a single stream [M, d]
def _attn_sublayer_fwd(blk, p, rt):
    h1, rstd1 = K.rmsnorm_fwd(p, blk.norm1.weight)
    ctx, att_saved = ops.attention_forward(blk.att, blk._arena, h1, rt)
    y = K.gemm(L.GEMM_NT, ctx, blk.att.out_proj.weight)
    return y, (h1, rstd1, ctx, att_saved)


def _attn_sublayer_bwd(blk, p, saved, dy, rt):
    arena, att = blk._arena, blk.att
    h1, rstd1, ctx, att_saved = saved
    wg = []
    fused = K.dgrad_attn_delta(dy, att.out_proj.weight, ctx, att_saved[4], rt.B, rt.S, att.num_heads, att.head_dim)
    dctx, delta = fused if fused is not None else (K.dgrad(dy, att.out_proj.weight), None)
    ops._wgrad(arena, att.out_proj.weight, None, dy, ctx, wg)
    dh1 = ops.attention_backward(att, arena, h1, ctx, att_saved, dctx, rt, wg, delta)
    gview, gacc = ops._vecgrad(arena, blk.norm1.weight)
    dp, _ = K.rmsnorm_bwd(p, blk.norm1.weight, rstd1, dh1, dw_out=gview, dw_accumulate=gacc)
    ops._flush_wgrads(wg)
    return dp


def _ffn_sublayer_fwd(blk, p, rt):
    arena, ffn = blk._arena, blk.ffn
    F_ = ffn.lin1.weight.shape[0]
    h2, rstd2 = K.rmsnorm_fwd(p, blk.norm2.weight)
    wgu = arena.fused(ffn.lin1.weight, ffn.lin_gate.weight)
    if ops.FUSE_SWIGLU_FWD and F_ % 32 == 0:
        gu, a = K.gemm_gateup_swiglu(h2, wgu)
    else:
        gu = K.gemm(L.GEMM_NT, h2, wgu)
        a = K.swiglu_fwd(gu, F_)
    y = K.gemm(L.GEMM_NT, a, ffn.lin2.weight)
    return y, (h2, rstd2, gu, a)


def _ffn_sublayer_bwd(blk, p, saved, dy, rt):
    arena, ffn = blk._arena, blk.ffn
    F_ = ffn.lin1.weight.shape[0]
    h2, rstd2, gu, a = saved
    wg = []
    if ops.FUSE_SWIGLU_BWD:
        dgu = K.gemm_dgrad_swiglu_bwd(dy, ffn.lin2.weight, gu)
    else:
        dgu = K.swiglu_bwd(gu, K.dgrad(dy, ffn.lin2.weight), F_)
    ops._wgrad(arena, ffn.lin2.weight, None, dy, a, wg)
    wgu = arena.fused(ffn.lin1.weight, ffn.lin_gate.weight)
    dh2 = K.dgrad(dgu, wgu)
    ops._wgrad(arena, ffn.lin1.weight, ffn.lin_gate.weight, dgu, h2, wg)
    gview, gacc = ops._vecgrad(arena, blk.norm2.weight)
    dp, _ = K.rmsnorm_bwd(p, blk.norm2.weight, rstd2, dh2, dw_out=gview, dw_accumulate=gacc)
    ops._flush_wgrads(wg)
    return dp


class _HCHalfFn(torch.autograd.Function):
    """One half of a block around its hyper-connections (hyper_qwen3.py:134-150 for attention, :153-164 for the FFN)."""

    @staticmethod
    def forward(ctx, x, blk, which, rt, keep, *params):
        hc, sub_fwd = (blk.hc_attn, _attn_sublayer_fwd) if which == "attn" else (blk.hc_ffn, _ffn_sublayer_fwd)
        B, S, n, d = x.shape
        x2 = x.reshape(B * S, n, d)
        x2 = x2 if x2.is_contiguous() else x2.contiguous()
        c = _coeffs(hc)
        r, p, h, th, rstd = KH.width_fwd(x2, c, eps=hc["norm"].eps)
        y, sub_saved = sub_fwd(blk, p, rt)
        out = KH.depth_fwd(y, h, r, out=r)  # in place: the backward does not need R (dR is dOut)
        ctx.blk, ctx.which, ctx.rt, ctx.shape = blk, which, rt, (B, S, n, d)
        ctx.saved = (x2, p, h, th, rstd, y, sub_saved) if keep else None
        return out.view(B, S, n, d)

    @staticmethod
    def backward(ctx, dout):
        if ctx.saved is None:
            raise RuntimeError("HyperQwen3TransformerBlock: backward through a forward that ran without grad mode")
        blk, (B, S, n, d) = ctx.blk, ctx.shape
        hc, sub_bwd = (blk.hc_attn, _attn_sublayer_bwd) if ctx.which == "attn" else (blk.hc_ffn, _ffn_sublayer_bwd)
        x2, p, h, th, rstd, y, sub_saved = ctx.saved
        dout2 = dout.reshape(B * S, n, d)
        dout2 = dout2 if dout2.is_contiguous() else dout2.contiguous()
        dy, dh_post = KH.depth_bwd(dout2, y, h)
        dp = sub_bwd(blk, p, sub_saved, dy, ctx.rt)
        dx, g = KH.width_bwd(dout2, dp, dh_post, x2, h, th, rstd, _coeffs(hc))
        _store_coeff_grads(blk, hc, g)
        ctx.saved = None
        return (dx.view(B, S, n, d), None, None, None, None) + (None,) * len(blk._param_list)


class HyperQwen3TransformerBlock(TransformerBlock):
    """Qwen3 block on n residual streams: x [B, S, n, emb] -> [B, S, n, emb].

    Parameters live in two arenas: the bf16 ones (attention, FFN, the four RMSNorm weights) in ``_arena`` like the plain block's, the 18
    fp32 coefficient tensors of the six connections in ``_hc_arena`` (an arena holds one dtype; the optimizer sees one buffer, not 18)."""

    def __init__(self, cfg, layer_idx, hc_type, expansion_rate=4):
        _check_hc_type(hc_type)
        super().__init__(cfg, layer_idx)
        self.hc_type = hc_type
        self.hc_attn = _create_hyper_connection_set(cfg["emb_dim"], expansion_rate, cfg["dtype"])
        self.hc_ffn = _create_hyper_connection_set(cfg["emb_dim"], expansion_rate, cfg["dtype"])

    def _build_arenas(self):
        """(Re)attach both arenas; ``ensure()`` rebuilds one whose parameters were moved or cast since the last forward."""
        if getattr(self, "_arena", None) is None:
            coeff_mods = [m for hc in (self.hc_attn, self.hc_ffn) for key in ("res", "pre", "post") for m in hc[key].modules()]
            named = list(self.named_parameters())
            coeff_ids = {id(p) for m in coeff_mods for p in m.parameters(recurse=False)}
            a16 = ParamArena([(k, p) for k, p in named if id(p) not in coeff_ids])
            a32 = ParamArena([(k, p) for k, p in named if id(p) in coeff_ids])
            for m in self.modules():
                object.__setattr__(m, "_arena", a16)
            for m in coeff_mods:
                object.__setattr__(m, "_arena", a32)
            object.__setattr__(self, "_hc_arena", a32)
            object.__setattr__(self, "_param_list", [p for _, p in named])
        self._arena.ensure()
        self._hc_arena.ensure()

    def forward(self, x, mask, cos, sin, attn_mask=None, kv_cache=None, position_ids=None, _runtime=None):
        if kv_cache is not None:
            raise NotImplementedError("HyperQwen3TransformerBlock: the KV-cache (inference) path over n streams is not implemented; pass kv_cache=None")
        L.require_gpu(x)
        if x.dim() != 4:
            raise ValueError(f"HyperQwen3TransformerBlock expects [B, S, n, emb] streams, got shape {tuple(x.shape)}")
        if x.dtype != BF16:
            raise TypeError(f"HyperQwen3TransformerBlock expects bf16 activations, got {x.dtype}")
        B, S, n, d = x.shape
        for hc in (self.hc_attn, self.hc_ffn):
            if hc["res"].linear.weight.shape[0] != n:
                raise ValueError(f"input has {n} streams, the block was built with expansion_rate={hc['res'].linear.weight.shape[0]}")
        self._build_arenas()
        rt = _runtime if _runtime is not None else ops.make_runtime(B, S, x.device, cos, sin, attn_mask, position_ids)
        keep = torch.is_grad_enabled()
        x = _HCHalfFn.apply(x, self, "attn", rt, keep, *self._param_list)
        return _HCHalfFn.apply(x, self, "ffn", rt, keep, *self._param_list)


class _StreamBroadcastFn(torch.autograd.Function):
    """x.unsqueeze(-2).expand(-1, -1, n, -1) (hyper_qwen3.py:201), materialised: the blocks write every stream."""

    @staticmethod
    def forward(ctx, x, n):
        B, S, d = x.shape
        x2 = x.reshape(B * S, d)
        ctx.shape = (B, S, n, d)
        return KH.stream_broadcast(x2 if x2.is_contiguous() else x2.contiguous(), n).view(B, S, n, d)

    @staticmethod
    def backward(ctx, dy):
        B, S, n, d = ctx.shape
        dy2 = dy.reshape(B * S, n, d)
        return KH.stream_sum(dy2 if dy2.is_contiguous() else dy2.contiguous()).view(B, S, d), None


class _StreamSumFn(torch.autograd.Function):
    """x.sum(dim=-2) (hyper_qwen3.py:224)."""

    @staticmethod
    def forward(ctx, x):
        B, S, n, d = x.shape
        x2 = x.reshape(B * S, n, d)
        ctx.shape = (B, S, n, d)
        return KH.stream_sum(x2 if x2.is_contiguous() else x2.contiguous()).view(B, S, d)

    @staticmethod
    def backward(ctx, dy):
        B, S, n, d = ctx.shape
        dy2 = dy.reshape(B * S, d)
        return KH.stream_broadcast(dy2 if dy2.is_contiguous() else dy2.contiguous(), n).view(B, S, n, d)


class HyperQwen3Model(Qwen3Model):
    """Dense Qwen3 with hyper-connections: embedding -> n copies -> blocks on n streams -> sum of the streams -> final norm -> head."""

    def __init__(self, cfg, hc_type, expansion_rate=4):
        _check_hc_type(hc_type)
        if cfg.get("gradient_checkpointing", False):
            raise NotImplementedError("HyperQwen3Model: gradient_checkpointing=True (recomputation of a block's activations) is not implemented")
        super().__init__(dict(cfg, n_layers=0))  # everything but the blocks: the plain blocks would be built only to be replaced
        self.expansion_rate = expansion_rate
        self.trf_blocks = nn.ModuleList(
            [HyperQwen3TransformerBlock(cfg, i, hc_type=hc_type, expansion_rate=expansion_rate) for i in range(cfg["n_layers"])]
        )

    def _build_arenas(self):
        if self._arenas_built:
            return
        for blk in self.trf_blocks:
            blk._build_arenas()
        top = [("emb_dict.weight", self.emb_dict.weight), ("final_norm.weight", self.final_norm.weight)]
        if not self.tie_embeddings:
            top.append(("out_head.weight", self.out_head.weight))
        ar = ParamArena(top)
        for m in (self.emb_dict, self.final_norm, self.out_head):
            object.__setattr__(m, "_arena", ar)
        object.__setattr__(self, "_top_arena", ar)
        self._arenas_built = True

    def arenas(self):
        """Gradient buffers in backward-completion order: per block (last first) its bf16 arena and its fp32 coefficient arena, then the top one."""
        self._build_arenas()
        out = []
        for blk in reversed(self.trf_blocks):
            out += [blk._arena, blk._hc_arena]
        return out + [self._top_arena]

    def _rope_tables(self):
        """The RoPE tables as the kernels take them, fp32.  ``model.to(torch.bfloat16)`` -- how the reference's training script builds this model -- casts
        the ``cos`` / ``sin`` buffers along with the parameters; the kernels multiply by bf16-rounded cos / sin anyway, so casting them back is lossless."""
        if self.cos.dtype == torch.float32:
            return self.cos, self.sin
        key = (self.cos.data_ptr(), self.sin.data_ptr())
        if getattr(self, "_rope_f32_key", None) != key:
            object.__setattr__(self, "_rope_f32", (K.cast(self.cos, torch.float32), K.cast(self.sin, torch.float32)))
            object.__setattr__(self, "_rope_f32_key", key)
        return self._rope_f32

    def forward_hidden(self, x, attn_mask=None, position_ids=None, input_embedded=False, keep_rows=None):
        """Blocks + final norm: (b, s) ids or (b, s, emb) embeddings -> (b, s, emb); ``keep_rows`` = (lo, hi) returns those rows of every sample."""
        if self.gradient_checkpointing:
            raise NotImplementedError("HyperQwen3Model: gradient_checkpointing=True (recomputation of a block's activations) is not implemented")
        L.require_gpu(x)
        self._build_arenas()
        if not input_embedded:
            x = self.emb_dict(x)
        elif x.dtype != self.emb_dict.weight.dtype:
            raise TypeError(f"embedded input must be {self.emb_dict.weight.dtype}, got {x.dtype}")
        B, S, _ = x.shape
        cos, sin = self._rope_tables()
        rt = ops.make_runtime(B, S, x.device, cos, sin, attn_mask, position_ids)
        x = _StreamBroadcastFn.apply(x, self.expansion_rate)
        for blk in self.trf_blocks:
            x = blk(x, self.mask, self.cos, self.sin, attn_mask, None, position_ids, _runtime=rt)
        x = _StreamSumFn.apply(x)
        if keep_rows is not None and tuple(keep_rows) != (0, S):
            x = x[:, int(keep_rows[0]) : int(keep_rows[1])]
        return self.final_norm(x)

    def forward(self, x, attn_mask=None, kv_cache=None, position_ids=None, input_embedded=False):
        """Logits (b, s, vocab) in the model dtype (reference: hyper_qwen3.py:190-229)."""
        if kv_cache is not None:
            raise NotImplementedError("HyperQwen3Model: the KV-cache (inference) path over n streams is not implemented; pass kv_cache=None")
        return self.out_head(self.forward_hidden(x, attn_mask, position_ids, input_embedded))
