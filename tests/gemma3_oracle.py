"""Plain-torch restatement of the Gemma3 arithmetic, written from the formulas of the kernels' contract (include/mi355_vlm.h,
csrc/attention_band.hip, csrc/gemma3.hip).  TEST INFRASTRUCTURE ONLY: one function per kernel, plus a block and a model.

Every function runs in one of two flows:
  * ``exact=False``: the reference's dtype flow -- bf16 tensors, every torch op rounding its result to bf16 where the reference's
    modules do (RMSNorm normalises in fp32, rounds, then multiplies by the scale in bf16; RoPE, LayerNorm, GELU, the score matrix,
    softmax and the weighted sum are bf16 ops).
  * ``exact=True``: fp64 throughout, no intermediate rounding -- the value every implementation is measured against.  The cos / sin
    tables are rounded to bf16 first in BOTH flows: that rounding is part of the function (``RoPE.apply`` casts them to x's dtype).
The backward functions differentiate the forward ones with autograd, as the reference does.

Attention operands are [B, H, S, D]; ``to_tokens`` / ``from_tokens`` convert to the kernels' token-major [B*S, H*D].
The window: key j is visible to query i iff i - W < j <= i (W >= S: plain causal).
"""

import glob
import math
import os

import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RMS_EPS, LN_EPS = 1e-6, 1e-5
BF16 = torch.bfloat16

TINY_GEMMA3 = dict(vocab_size=512, context_length=96, emb_dim=128, n_heads=2, num_kv_groups=1, n_layers=3, hidden_dim=256, window_size=40,
                   local_global_att_ratio=2, rope_base=10000, dtype=torch.bfloat16)


def _c(t, exact):
    return t.double() if exact else t


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def to_tokens(x):
    """[B, H, S, D] -> [B*S, H*D]"""
    B, H, S, D = x.shape
    return x.transpose(1, 2).reshape(B * S, H * D).contiguous()


def from_tokens(x, B, S, H, D):
    return x.reshape(B, S, H, D).transpose(1, 2)


# ----------------------------------------------------------------------------------------------------------------- kernels
def band_mask(S, W):
    """bool [S, S], True = masked: not (i - W < j <= i)."""
    i = torch.arange(S).unsqueeze(1)
    j = torch.arange(S).unsqueeze(0)
    return ~((j <= i) & (j > i - W))


def swa_attention(q, k, v, W, exact=False, scale=None):
    """q [B, Hq, S, D], k / v [B, Hkv, S, D] -> (o [B, Hq, S, D], lse [B, Hq, S]): the band mask on the full score matrix."""
    B, Hq, S, D = q.shape
    rep = Hq // k.shape[1]
    scale = D ** -0.5 if scale is None else scale
    q, k, v = _c(q, exact), _c(k, exact), _c(v, exact)
    k, v = k.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1)
    s = (q @ k.mT) * scale
    s = s.masked_fill(band_mask(S, W), -torch.inf)
    p = F.softmax(s, dim=-1)
    return p @ v, torch.logsumexp(s.double() if exact else s.float(), dim=-1)


def swa_attention_bwd(q, k, v, do, W, exact=False, scale=None):
    """-> (dq, dk, dv) by autograd."""
    qg, kg, vg = [_c(t, exact).detach().requires_grad_(True) for t in (q, k, v)]
    o, _ = swa_attention(qg, kg, vg, W, exact, scale)
    return torch.autograd.grad(o, [qg, kg, vg], _c(do, exact))


def swa_attention_gather(q, k, v, W, scale=None):
    """The reference's semantics in its own form: every query against the W keys ending at itself, positions before the sequence start padded
    and masked (independent of the band mask above: tests compare the two).  fp64.  q, k, v [B, H, S, D], same H."""
    B, H, S, D = q.shape
    scale = D ** -0.5 if scale is None else scale
    q, k, v = q.double(), k.double(), v.double()
    out = torch.zeros_like(q)
    for i in range(S):
        lo = max(0, i - W + 1)
        s = (q[:, :, i : i + 1] @ k[:, :, lo : i + 1].mT) * scale
        out[:, :, i : i + 1] = F.softmax(s, dim=-1) @ v[:, :, lo : i + 1]
    return out


def rmsnorm(x, scale, residual=None, exact=False):
    """scale * x / (sqrt(mean(x^2)) + eps) [+ residual]: eps is added to the RMS."""
    if exact:
        x = x.double()
        y = scale.double() * (x / (torch.sqrt(torch.mean(x ** 2, dim=-1, keepdim=True)) + RMS_EPS))
        return y if residual is None else y + residual.double()
    xf = x.to(torch.float32)
    norm = xf / (torch.sqrt(torch.mean(xf ** 2, dim=-1, keepdim=True)) + RMS_EPS)
    y = scale * norm.to(x.dtype)
    return y if residual is None else y + residual


def rmsnorm_bwd(x, scale, dy, exact=False):
    """-> (dx, dscale) by autograd (no residual: its gradient is dy itself)."""
    xg, sg = [_c(t, exact).detach().requires_grad_(True) for t in (x, scale)]
    return torch.autograd.grad(rmsnorm(xg, sg, None, exact), [xg, sg], _c(dy, exact))


def rope(x, cos, sin, exact=False):
    """x [B, H, S, D]; cos / sin fp32 [>= S, D]: cos * x + sin * cat(-x2, x1) with cos / sin rounded to bf16."""
    S, D = x.shape[-2], x.shape[-1]
    c, s = cos[:S].to(BF16), sin[:S].to(BF16)
    c, s = (c.double(), s.double()) if exact else (c.to(x.dtype), s.to(x.dtype))
    rot = torch.cat((-x[..., D // 2 :], x[..., : D // 2]), dim=-1)
    return c * x + s * rot


def layernorm(x, scale, shift, exact=False):
    """(x - mean) / (std + eps) * scale + shift over the last dim, population std."""
    std = torch.std(x, dim=-1, keepdim=True, unbiased=False)
    mean = x.mean(dim=-1, keepdim=True)
    return scale * ((x - mean) / (std + LN_EPS)) + shift


def rope_ln(x, cos, sin, scale, shift, exact=False):
    """RoPE then per-head LayerNorm on x [B, H, S, D]."""
    x, scale, shift = _c(x, exact), _c(scale, exact), _c(shift, exact)
    return layernorm(rope(x, cos, sin, exact), scale, shift, exact)


def rope_ln_bwd(x, cos, sin, scale, shift, dy, exact=False):
    """-> (dx, dscale, dshift) by autograd."""
    xg, sg, bg = [_c(t, exact).detach().requires_grad_(True) for t in (x, scale, shift)]
    return torch.autograd.grad(rope_ln(xg, cos, sin, sg, bg, exact), [xg, sg, bg], _c(dy, exact))


def gelu(x):
    return x * 0.5 * (1 + torch.erf(x / math.sqrt(2)))


def geglu(gu, exact=False):
    """gu [T, 2F] = [lin1 | lin_gate] -> lin1 * gelu_erf(lin_gate)."""
    gu = _c(gu, exact)
    Fh = gu.shape[-1] // 2
    return gu[..., :Fh] * gelu(gu[..., Fh:])


def geglu_bwd(gu, da, exact=False):
    g = _c(gu, exact).detach().requires_grad_(True)
    return torch.autograd.grad(geglu(g, exact), [g], _c(da, exact))[0]


# ----------------------------------------------------------------------------------------------------------------- block and model
def rope_tables(base, head_dim, ctx):
    """cos / sin fp32 [ctx, head_dim]: angle of position m, feature i is m * base^(-2 (i mod D/2) / D)."""
    inv = 1.0 / base ** (2 * torch.arange(0, head_dim // 2, dtype=torch.float32) / head_dim)
    ang = torch.outer(torch.arange(0, ctx, dtype=torch.float32), inv)
    ang = torch.cat((ang, ang), dim=-1)
    return torch.cos(ang), torch.sin(ang)


def is_windowed(cfg, layer):
    return cfg["window_size"] > 0 and (layer + 1) % (cfg["local_global_att_ratio"] + 1) != 0


def attention_core(sd, pfx, x, cfg, layer, cos, sin, exact=False, capture=None):
    """GroupedQueryAttention up to (not including) out_proj: x [b, s, d] -> context [b, s, d]."""
    b, s, _ = x.shape
    Hq, Hkv = cfg["n_heads"], cfg["num_kv_groups"]
    D = cfg["emb_dim"] // Hq
    w = lambda k: _c(sd[pfx + k], exact)
    q = F.linear(x, w("w_queries.weight")).view(b, s, Hq, D).transpose(1, 2)
    k = F.linear(x, w("w_keys.weight")).view(b, s, Hkv, D).transpose(1, 2)
    v = F.linear(x, w("w_values.weight")).view(b, s, Hkv, D).transpose(1, 2)
    q = rope_ln(q, cos, sin, w("q_norm.scale"), w("q_norm.shift"), exact)
    k = rope_ln(k, cos, sin, w("k_norm.scale"), w("k_norm.shift"), exact)
    W = cfg["window_size"] if is_windowed(cfg, layer) else s
    o, _ = swa_attention(q, k, v, W, exact)
    if capture is not None:
        capture.update(q=q, k=k, v=v, ctx=o)
    return o.transpose(1, 2).reshape(b, s, Hq * D)


def block(sd, pfx, x, cfg, layer, cos, sin, exact=False, capture=None):
    """TransformerBlock.forward on x [b, s, d]; ``capture`` (a dict) receives q, k, v, ctx, the input / output of post_att_norm and the FFN's
    gated product."""
    w = lambda k: _c(sd[pfx + k], exact)
    res = x
    h = rmsnorm(x, w("pre_att_norm.scale"), None, exact)
    ctx = attention_core(sd, pfx + "att.", h, cfg, layer, cos, sin, exact, capture)
    ao = F.linear(ctx, w("att.out_proj.weight"), w("att.out_proj.bias"))
    pn = rmsnorm(ao, w("post_att_norm.scale"), None, exact)
    x = pn + res
    res = x
    h = rmsnorm(x, w("pre_ffn_norm.scale"), None, exact)
    up, pre = F.linear(h, w("ffn.lin1.weight")), F.linear(h, w("ffn.lin_gate.weight"))
    prod = up * gelu(pre)
    f = F.linear(prod, w("ffn.lin2.weight"))
    if capture is not None:
        capture.update(post_att_in=ao, post_att_out=pn, ffn_prod=prod, ffn_up=up, ffn_gate=pre)
    return rmsnorm(f, w("post_ffn_norm.scale"), None, exact) + res


def model(sd, cfg, ids, exact=False, capture_block=None, capture=None):
    """Gemma3Model.forward: logits [b, s, vocab]."""
    D = cfg["emb_dim"] // cfg["n_heads"]
    cos, sin = rope_tables(cfg["rope_base"], D, cfg["context_length"])
    x = _c(F.embedding(ids, sd["emb_dict.weight"]), exact)
    for i in range(cfg["n_layers"]):
        x = block(sd, f"trf_blocks.{i}.", x, cfg, i, cos, sin, exact, capture if i == capture_block else None)
    x = rmsnorm(x, _c(sd["final_norm.scale"], exact), None, exact)
    return F.linear(x, _c(sd["emb_dict.weight"], exact))


# ----------------------------------------------------------------------------------------------------------------- fixture and operands
def load_fixture():
    """tests/golden/gemma3_tiny.safetensors and its .partK continuation files (every committed file stays under 1 MiB) as one dict."""
    from safetensors.torch import load_file

    t = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, "gemma3_tiny*.safetensors"))):
        t.update(load_file(path))
    if not t:
        raise FileNotFoundError("tests/golden/gemma3_tiny*.safetensors")
    return t


def perturb_parameters(named_parameters, gen):
    """The fixture recipe: emb_dict.weight ~ N(0, 0.05); every norm scale / shift and out_proj.bias moved off its initial value by
    0.1 * N(0, 1), drawn in parameter order from ``gen``."""
    with torch.no_grad():
        for k, p in named_parameters:
            if k == "emb_dict.weight":
                p.copy_((torch.randn(p.shape, generator=gen) * 0.05).to(p.dtype))
            elif k.endswith((".scale", ".shift", "out_proj.bias")):
                p.add_((0.1 * torch.randn(p.shape, generator=gen)).to(p.dtype))


def attn_operands(B, S, Hq, Hkv, D, seed):
    """q, k, v, do as bf16 [B, H, S, D], N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda h: torch.randn(B, h, S, D, generator=g).to(BF16)
    return rn(Hq), rn(Hkv), rn(Hkv), rn(Hq)


def row_operands(T, d, seed):
    """x, dy, residual bf16 [T, d]; scale bf16 [d] = 1 + 0.1 N(0, 1).  Rows are scaled by powers of two from 1/8 to 8 in turn."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, d, generator=g) * (2.0 ** ((torch.arange(T) % 7) - 3)).unsqueeze(1)
    dy = torch.randn(T, d, generator=g)
    res = torch.randn(T, d, generator=g)
    scale = 1.0 + 0.1 * torch.randn(d, generator=g)
    return x.to(BF16), dy.to(BF16), res.to(BF16), scale.to(BF16)


def rope_ln_operands(B, S, H, D, seed):
    """x, dy bf16 [B, H, S, D]; (scale, shift) bf16 [D] off their initial values."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, S, D, generator=g).to(BF16)
    dy = torch.randn(B, H, S, D, generator=g).to(BF16)
    scale = (1.0 + 0.1 * torch.randn(D, generator=g)).to(BF16)
    shift = (0.1 * torch.randn(D, generator=g)).to(BF16)
    return x, dy, scale, shift


def geglu_operands(T, Fh, seed):
    """gu bf16 [T, 2F] with gate values spanning [-8, 8] (every row sweeps the range), da bf16 [T, F]."""
    g = torch.Generator().manual_seed(seed)
    up = torch.randn(T, Fh, generator=g)
    gate = torch.linspace(-8.0, 8.0, Fh).repeat(T, 1) + 0.05 * torch.randn(T, Fh, generator=g)
    da = torch.randn(T, Fh, generator=g)
    return torch.cat((up, gate), dim=1).to(BF16), da.to(BF16)
