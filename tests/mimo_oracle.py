"""Plain-torch restatement of the MiMo-V2-Flash arithmetic, written from the formulas of the kernels' contract (include/mi355_vlm.h,
csrc/attention_band.hip, csrc/mimo.hip): attention with a sink and its own value head dim, the per-head RMSNorm + partial RoPE, the block and the model with its MTP
modules.  TEST INFRASTRUCTURE ONLY.  The mixture-of-experts layer is tests/deepseek_moe_oracle.py's (0 shared experts).

Every function runs in one of two flows:
  * ``exact=False``: the reference's dtype flow -- bf16 tensors, every torch op rounding its result to bf16 where the reference's modules do
    (the score matrix, the concatenation with the sink column, the softmax and the weighted sum are bf16 ops; RMSNorm runs in fp32 and is
    rounded once; RoPE is a bf16 op);
  * ``exact=True``: fp64 throughout, no intermediate rounding -- the value every implementation is measured against.  The cos / sin tables
    are rounded to bf16 first in BOTH flows: that rounding is part of the function (``RoPE.apply`` casts them to x's dtype).
The backward functions differentiate the forward ones with autograd, as the reference does.

Attention operands are [B, H, S, D] (v and o: DV wide); ``to_tokens`` / ``from_tokens`` convert to the kernels' token-major layout.
The window: key j is visible to query i iff i - W < j <= i (W >= S: plain causal).  ``sink``: [Hq] logits or None.
"""

import torch
import torch.nn.functional as F

import deepseek_moe_oracle as MO
from gemma3_oracle import GOLDEN, band_mask, from_tokens, rel_l2, to_tokens  # noqa: F401

BF16 = torch.bfloat16
RMS_EPS = 1e-6

# every branch of the model: GA-dense, SWA-MoE, GA-MoE, SWA-MoE; GQA ratios 3 (SWA) and 6 (GA); D != DV; R = 20 of 64; two MTP modules
TINY_MIMO = dict(vocab_size=256, context_length=96, emb_dim=128, n_layers=4, n_heads=6, num_swa_kv_groups=2, num_ga_kv_groups=1, head_dim=64,
                 value_head_dim=32, hidden_dim=32, window_size=24, hybrid_ratio=3, rope_base=10_000, rope_base_ga=640_000, partial_rope_factor=0.33,
                 mtp_depth=2, mtp_loss_coeff=0.3, num_experts=8, top_k=2, num_shared_experts=0, moe_scaling_factor=1.0, moe_bias_update_rate=1e-3,
                 dtype=torch.bfloat16)
FIXTURE_BATCH, FIXTURE_SEQ = 2, 70
# gradients whose floor (the reference's own bf16-vs-fp32 distance) may exceed 0.1, by name suffix, with the reason; tools/gen_golden_mimo.py
# checks the list against the reference's numbers.  Empty: on the fixture every floor is below 0.1 (the worst is 0.055)
FLOOR_ALLOW = {}


def floor_allowed(name):
    return name.endswith(tuple(FLOOR_ALLOW))


def _c(t, exact):
    return t.double() if exact else t


def is_swa(cfg, layer):
    return layer > 0 and (layer + 1) % cfg["hybrid_ratio"] != 0


def is_moe(cfg, layer):
    return layer > 0


def moe_layers(cfg):
    return [i for i in range(cfg["n_layers"]) if is_moe(cfg, i)]


def load_fixture(stem="mimo_tiny"):
    return MO.load_fixture(stem)


# ----------------------------------------------------------------------------------------------------------------- kernels
def sink_attention(q, k, v, W, sink=None, exact=False, scale=None):
    """q [B, Hq, S, D], k [B, Hkv, S, D], v [B, Hkv, S, DV], sink [Hq] or None -> (o [B, Hq, S, DV], lse [B, Hq, S], the sink included)."""
    B, Hq, S, D = q.shape
    rep = Hq // k.shape[1]
    scale = D ** -0.5 if scale is None else scale
    q, k, v = _c(q, exact), _c(k, exact), _c(v, exact)
    k, v = k.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1)
    s = (q @ k.mT) * scale
    s = s.masked_fill(band_mask(S, W), -torch.inf)
    if sink is not None:
        s = torch.cat([s, _c(sink, exact).to(s.dtype).view(1, Hq, 1, 1).expand(B, -1, S, -1)], dim=-1)
    p = F.softmax(s, dim=-1)
    lse = torch.logsumexp(s.double() if exact else s.float(), dim=-1)
    if sink is not None:
        p = p[..., :-1]
    return p @ v, lse


def sink_attention_bwd(q, k, v, do, W, sink=None, exact=False, scale=None):
    """-> (dq, dk, dv, dsink) by autograd; dsink is None without a sink."""
    leaves = [_c(t, exact).detach().requires_grad_(True) for t in (q, k, v)]
    zg = None if sink is None else _c(sink, exact).detach().requires_grad_(True)
    o, _ = sink_attention(*leaves, W, zg, exact, scale)
    g = torch.autograd.grad(o, leaves + ([] if zg is None else [zg]), _c(do, exact))
    return g[0], g[1], g[2], (None if zg is None else g[3])


def dsink_formula(sink, lse, delta):
    """dz[h] = - sum_{b,i} exp(z_h - lse[b,h,i]) * delta[b,h,i], in the operands' dtype (what mi355_sink_attn_bwd's sink pass computes)."""
    return -(torch.exp(sink.view(1, -1, 1) - lse) * delta).sum(dim=(0, 2))


def rms_norm(x, weight, exact=False, eps=RMS_EPS):
    """PytorchRMSNorm: torch's RMSNorm (eps under the root) on the fp32 cast, rounded back to x's dtype."""
    if exact:
        x = x.double()
        return x * torch.rsqrt(x.pow(2).mean(dim=-1, keepdim=True) + eps) * weight.double()
    xf = x.to(torch.float32)  # torch.rms_norm on an fp32 input with a bf16 weight takes its composite path: these ops, the product with the weight in fp32
    return ((xf * torch.rsqrt(xf.pow(2).mean(dim=-1, keepdim=True) + eps)) * weight).to(x.dtype)


def partial_rope(x, cos, sin, exact=False):
    """x [B, H, S, D]; cos / sin [>= S, R], R <= D: the half-split rotation of the first R features with cos / sin rounded to bf16; the rest pass."""
    S, R = x.shape[-2], cos.shape[-1]
    c, s = cos[:S].to(BF16), sin[:S].to(BF16)
    c, s = (c.double(), s.double()) if exact else (c.to(x.dtype), s.to(x.dtype))
    head, rest = x[..., :R], x[..., R:]
    rot = torch.cat((-head[..., R // 2 :], head[..., : R // 2]), dim=-1)
    return torch.cat((c * head + s * rot, rest), dim=-1)


def norm_rope(x, weight, cos, sin, exact=False):
    """Per-head RMSNorm then partial RoPE on x [B, H, S, D]."""
    return partial_rope(rms_norm(_c(x, exact), _c(weight, exact), exact), cos, sin, exact)


def norm_rope_bwd(x, weight, cos, sin, dy, exact=False):
    """-> (dx, dweight) by autograd."""
    xg, wg = [_c(t, exact).detach().requires_grad_(True) for t in (x, weight)]
    return torch.autograd.grad(norm_rope(xg, wg, cos, sin, exact), [xg, wg], _c(dy, exact))


# ----------------------------------------------------------------------------------------------------------------- block and model
def rope_tables(base, head_dim, ctx, rotation_factor):
    """cos / sin fp32 [ctx, R]: with r = int(head_dim * rotation_factor) (21 for 64 and 0.33) there are r // 2 frequencies base^(-2 i / r) -- r itself,
    odd or not, stays in the exponent -- and R = 2 (r // 2) rotated features; angle of position m, feature i is m * base^(-2 (i mod R/2) / r)."""
    r = int(head_dim * rotation_factor) if rotation_factor != 1.0 else head_dim
    inv = 1.0 / base ** (2 * torch.arange(0, r // 2, dtype=torch.float32) / r)
    ang = torch.outer(torch.arange(0, ctx, dtype=torch.float32), inv)
    ang = torch.cat((ang, ang), dim=-1)
    return torch.cos(ang), torch.sin(ang)


def tables(cfg):
    """{True: (cos_swa, sin_swa), False: (cos_ga, sin_ga)}"""
    mk = lambda base: rope_tables(base, cfg["head_dim"], cfg["context_length"], cfg["partial_rope_factor"])
    return {True: mk(cfg.get("rope_base", 10000)), False: mk(cfg.get("rope_base_ga", 640000))}


def attention(sd, pfx, x, cfg, swa, cos, sin, exact=False, capture=None):
    """GroupedQueryAttentionWithSink.forward on x [b, s, d] (out_proj included)."""
    b, s, _ = x.shape
    Hq, Hkv = cfg["n_heads"], cfg["num_swa_kv_groups" if swa else "num_ga_kv_groups"]
    D = cfg["head_dim"]
    DV = cfg.get("value_head_dim") or D
    w = lambda k: _c(sd[pfx + k], exact)
    q = F.linear(x, w("w_queries.weight")).view(b, s, Hq, D).transpose(1, 2)
    k = F.linear(x, w("w_keys.weight")).view(b, s, Hkv, D).transpose(1, 2)
    v = F.linear(x, w("w_values.weight")).view(b, s, Hkv, DV).transpose(1, 2)
    q = norm_rope(q, w("q_norm.weight"), cos, sin, exact)
    k = norm_rope(k, w("k_norm.weight"), cos, sin, exact)
    o, _ = sink_attention(q, k, v, cfg["window_size"] if swa else s, w("sink") if swa else None, exact)
    if capture is not None:
        capture.update(q=q, k=k, v=v, ctx=o)
    return F.linear(o.transpose(1, 2).reshape(b, s, Hq * DV), w("out_proj.weight"))


def ffn(sd, pfx, x, exact=False):
    w = lambda k: _c(sd[pfx + k], exact)
    return F.linear(F.linear(x, w("lin1.weight")) * F.silu(F.linear(x, w("lin_gate.weight"))), w("lin2.weight"))


def block(sd, pfx, x, cfg, swa, moe, cos, sin, exact=False, idx=None, record=None, capture=None):
    """TransformerBlock.forward on x [b, s, d]."""
    w = lambda k: _c(sd[pfx + k], exact)
    x = _c(x, exact)
    x = attention(sd, pfx + "att.", rms_norm(x, w("norm1.weight"), exact), cfg, swa, cos, sin, exact, capture) + x
    h = rms_norm(x, w("norm2.weight"), exact)
    if moe:
        out, _ = MO.moe_layer(sd, pfx + "feed_forward.", h.reshape(-1, h.shape[-1]), cfg, torch.float64 if exact else None, idx, record)
        return out.view_as(x) + x
    return ffn(sd, pfx + "feed_forward.", h, exact) + x


def main_model(sd, cfg, ids, exact=False, idxs=None, records=None, captures=None):
    """MainModel.forward: (logits, h_final).  ``idxs`` / ``records`` / ``captures``: per layer number a forced selection / dicts to fill."""
    tb = tables(cfg)
    pfx = "main_model."
    x = _c(F.embedding(ids, sd[pfx + "emb_layer.weight"]), exact)
    for i in range(cfg["n_layers"]):
        swa = is_swa(cfg, i)
        x = block(sd, f"{pfx}layers.{i}.", x, cfg, swa, is_moe(cfg, i), *tb[swa], exact, None if idxs is None else idxs.get(i),
                  None if records is None else records.setdefault(i, {}), None if captures is None else captures.setdefault(i, {}))
    logits = F.linear(rms_norm(x, _c(sd[pfx + "final_norm.weight"], exact), exact), _c(sd[pfx + "out_head.weight"], exact))
    return logits, x


def model_loss(sd, cfg, ids, targets, exact=False, idxs=None, records=None):
    """MiMoModel.forward in training mode: (total loss, main logits).  MTP step k runs on the sliced sequence of length s - k - 1 with the SWA
    tables from position 0, its targets are the INPUT ids shifted by k + 1."""
    logits, h_prev = main_model(sd, cfg, ids, exact, idxs, records)
    loss = F.cross_entropy(logits.flatten(0, 1), targets.flatten())
    depth = cfg.get("mtp_depth", 0)
    if depth == 0:
        return loss, logits
    cos, sin = tables(cfg)[True]
    emb = _c(F.embedding(ids, sd["main_model.emb_layer.weight"]), exact)
    head = _c(sd["main_model.out_head.weight"], exact)
    extra = 0
    for i in range(depth):
        k, pfx = i + 1, f"mtp_modules.{i}."
        w = lambda name: _c(sd[pfx + name], exact)
        xs, tgt = emb[:, k:-1], ids[:, k + 1 :]
        hs = h_prev[:, :-2] if k == 1 else h_prev[:, :-1]
        x = F.linear(torch.cat([rms_norm(xs, w("rms_input.weight"), exact), rms_norm(hs, w("rms_h_prev.weight"), exact)], dim=-1), w("down_proj.weight"))
        h_prev = block(sd, pfx + "trf_block.", x, cfg, True, False, cos, sin, exact)
        lk = F.linear(rms_norm(h_prev, w("final_norm.weight"), exact), head)
        extra = extra + F.cross_entropy(lk.flatten(0, 1), tgt.flatten())
    return loss + (cfg["mtp_loss_coeff"] / depth) * extra, logits


# ----------------------------------------------------------------------------------------------------------------- fixture recipe and operands
def perturb_parameters(named_parameters, gen):
    """The fixture recipe: embedding ~ N(0, 0.05); every norm weight (the 1-D ``.weight`` parameters) and the gates' biases moved off their initial
    values by 0.1 * N(0, 1); every sink redrawn from 0.5 * N(0, 1) (upstream's 0.02 would leave it without weight in the softmax); drawn in
    parameter order from ``gen``."""
    with torch.no_grad():
        for k, p in named_parameters:
            if k.endswith("emb_layer.weight"):
                p.copy_((torch.randn(p.shape, generator=gen) * 0.05).to(p.dtype))
            elif k.split(".")[-1] == "sink":
                p.copy_((0.5 * torch.randn(p.shape, generator=gen)).to(p.dtype))
            elif p.dim() == 1 and k.endswith((".weight", ".bias")):
                p.add_((0.1 * torch.randn(p.shape, generator=gen)).to(p.dtype))



def attn_operands(B, S, Hq, Hkv, D, DV, seed, sink=True):
    """q, k [.., D], v, do [.., DV] as bf16 [B, H, S, .], N(0, 1); sink bf16 [Hq] ~ N(0, 1) (large against the reference's init, so that it weighs) or None."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda h, d: torch.randn(B, h, S, d, generator=g).to(BF16)
    q, k, v, do = rn(Hq, D), rn(Hkv, D), rn(Hkv, DV), rn(Hq, DV)
    return q, k, v, do, (torch.randn(Hq, generator=g).to(BF16) if sink else None)


def norm_rope_operands(B, S, H, D, seed):
    """x, dy bf16 [B, H, S, D] (rows scaled by powers of two from 1/8 to 8 in turn); weight bf16 [D] = 1 + 0.1 N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, S, D, generator=g) * (2.0 ** ((torch.arange(S) % 7) - 3)).view(1, 1, S, 1)
    dy = torch.randn(B, H, S, D, generator=g)
    return x.to(BF16), dy.to(BF16), (1.0 + 0.1 * torch.randn(D, generator=g)).to(BF16)
