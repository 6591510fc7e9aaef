"""Plain-torch restatement of the Llama 3.2 arithmetic and of QK-Clip: one function per kernel of csrc/llama3.hip (the fused RoPE and its
adjoint, the per-head maximum attention logit, the weight clip) plus attention, block and model, written from the formulas of the kernels' contract
(include/mi355_vlm.h).  TEST INFRASTRUCTURE ONLY.

Every function runs in one of two flows:
  * ``exact=False``: the reference's dtype flow on the tensors as given -- for bf16 tensors every torch op rounds its result to bf16 where the
    reference's modules do (RMSNorm normalises in fp32, rounds, then multiplies by the scale; the Linears, RoPE, the score matrix -- a bf16 matmul
    scaled in bf16 --, the softmax, the weighted sum and SiLU are bf16 ops); for fp32 tensors (the twin's weights) the same ops in fp32;
  * ``exact=True``: everything upcast to fp64 first, no intermediate rounding -- the value every implementation is measured against.
The cos / sin tables are rounded to bf16 first in EVERY flow: that rounding is part of the function (``RoPE.apply`` casts the tables to x's dtype,
the model's ``.to(bfloat16)`` rounds the buffers themselves, and the fixture's fp32 twin runs on the rounded tables).

Attention operands are [B, H, S, D]; ``to_tokens`` / ``from_tokens`` convert to the kernels' token-major form.  A key mask is bool / uint8 [B, S],
non-zero = a real token.
"""

import glob
import os

import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RMS_EPS = 1e-6
BF16, F64 = torch.bfloat16, torch.float64

TINY_LLAMA = dict(vocab_size=512, context_length=64, emb_dim=256, n_heads=4, num_kv_groups=2, n_layers=2, hidden_dim=512, rope_base=500_000,
                  dtype=torch.bfloat16)
FIXTURE_TAU = 4.0  # the threshold of the fixture's three clipped weight sets


def _c(t, exact):
    return t.to(F64) if exact else t


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
def rope_tables(base, dim, ctx):
    """cos / sin fp32 [ctx, dim]: angle of position m, feature i is m * base^(-2 (i mod dim/2) / dim)."""
    inv = 1.0 / base ** (2 * torch.arange(0, dim // 2, dtype=torch.float32) / dim)
    ang = torch.outer(torch.arange(0, ctx, dtype=torch.float32), inv)
    ang = torch.cat((ang, ang), dim=-1)
    return torch.cos(ang), torch.sin(ang)


def rope(x, cos, sin, pos=None, exact=False):
    """x [B, H, S, D]; cos / sin [rows, D]; pos None (the first S rows) or integer [B, S]: cos * x + sin * cat(-x2, x1), tables through bf16."""
    x = _c(x, exact)
    S, D = x.shape[-2], x.shape[-1]
    if pos is None:
        c, s = cos[:S], sin[:S]
    else:
        c, s = cos[pos.long()].unsqueeze(1), sin[pos.long()].unsqueeze(1)
    c, s = c.to(BF16).to(x.dtype), s.to(BF16).to(x.dtype)
    rot = torch.cat((-x[..., D // 2 :], x[..., : D // 2]), dim=-1)
    return c * x + s * rot


def rope_packed_fwd(qkv, cos, sin, pos, B, S, Hq, Hkv, D, exact=False):
    """mi355_llama_rope_fwd: qkv [B*S, (Hq + 2 Hkv) D] token-major, pos integer [B*S] -> (q [B*S, Hq D], k [B*S, Hkv D])."""
    p = pos.reshape(B, S)
    q = rope(from_tokens(qkv[:, : Hq * D], B, S, Hq, D), cos, sin, p, exact)
    k = rope(from_tokens(qkv[:, Hq * D : (Hq + Hkv) * D], B, S, Hkv, D), cos, sin, p, exact)
    return to_tokens(q), to_tokens(k)


def rope_packed_bwd(dq, dk, cos, sin, pos, B, S, Hq, Hkv, D, exact=False):
    """mi355_llama_rope_bwd: the adjoint rotation of dq, dk -> [B*S, (Hq + Hkv) D] (autograd through ``rope_packed_fwd`` at zero)."""
    z = torch.zeros(B * S, (Hq + 2 * Hkv) * D, dtype=F64 if exact else dq.dtype).requires_grad_(True)
    q, k = rope_packed_fwd(z, cos, sin, pos, B, S, Hq, Hkv, D, exact)
    (g,) = torch.autograd.grad([q, k], [z], [_c(dq, exact), _c(dk, exact)])
    return g[:, : (Hq + Hkv) * D]


def visible(B, S, key_mask=None):
    """bool [B, 1, S, S]: pair (i, j) is visible iff j <= i and key j of the sample is a real token."""
    vis = torch.ones(S, S, dtype=torch.bool).tril_().view(1, 1, S, S).expand(B, 1, S, S)
    if key_mask is not None:
        vis = vis & key_mask.bool().view(B, 1, 1, S)
    return vis


def scores(q, k, scale=None, exact=False):
    """q [B, Hq, S, D], k [B, Hkv, S, D] -> scale * q k^T [B, Hq, S, S]: a matmul and a multiplication in the operands' dtype (or fp64)."""
    q, k = _c(q, exact), _c(k, exact)
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    return (q @ k.repeat_interleave(q.shape[1] // k.shape[1], dim=1).mT) * scale


def max_logit(q, k, scale=None, key_mask=None, exact=False):
    """mi355_attn_max_logit: the maximum of the visible scores of every query head over batch, query and key, [Hq]; -inf without a visible pair,
    NaN if a visible score is NaN (torch.amax)."""
    s = scores(q, k, scale, exact)
    B, _, S, _ = s.shape
    s = torch.where(visible(B, S, key_mask), s, torch.full((), -torch.inf, dtype=s.dtype))
    return torch.amax(s, dim=(0, 2, 3)) if s.numel() else torch.full((q.shape[1],), -torch.inf, dtype=s.dtype)


def clip_gammas(m, tau, mode):
    """gamma per query head, fp32 [Hq], 1 = no clip.  A maximum that is NaN, infinite or not positive never clips (mode "naive": a NaN anywhere
    leaves the layer alone)."""
    m = m.float()
    one = torch.ones_like(m)
    if mode == "naive":
        top = torch.amax(m)  # NaN if any head is NaN
        ok = (top > tau) & (top > 0) & torch.isfinite(top)
        return torch.where(ok, tau / top, one[0]).expand_as(m).clone()
    v = m.abs() if mode == "magnitude" else m
    ok = (v > tau) & (v > 0) & torch.isfinite(v)
    return torch.where(ok, tau / v, one)


def qk_clip(wq, wk, m, Hq, Hkv, tau, alpha=0.5, mode="per_head"):
    """mi355_qk_clip out of place: (wq', wk') with w' = bf16(float(w) * s) on the head blocks that clip, the others untouched."""
    if mode == "magnitude" and Hq != Hkv:
        raise ValueError("the magnitude mode is defined for multi-head attention only")
    g = clip_gammas(m, tau, mode)
    gk = g.view(Hkv, Hq // Hkv).min(dim=1).values
    sq, sk = g ** alpha, gk ** (1 - alpha)
    out = []
    for w, s, H, gam in ((wq, sq, Hq, g), (wk, sk, Hkv, gk)):
        w3 = w.view(H, w.shape[0] // H, w.shape[1])
        scaled = (w3.float() * s.view(H, 1, 1)).to(w.dtype)
        out.append(torch.where((gam < 1).view(H, 1, 1), scaled, w3).reshape(w.shape))
    return out[0], out[1]


def clip_mismatches(before, got, want, heads):
    """How a clipped matrix ``got`` differs from the reference's ``want`` (both from ``before``), head block by head block: a head the reference left
    alone must be ``before`` bit for bit, any other within one bf16 step per element (the power gamma^alpha may differ in its last fp32 bit).  Returns
    the list of offending heads with the reason."""
    bad = []
    b3, g3, w3 = (x.detach().cpu().view(heads, -1, x.shape[1]) for x in (before, got, want))
    for h in range(heads):
        if torch.equal(w3[h], b3[h]):
            if not torch.equal(g3[h], b3[h]):
                bad.append(f"head {h}: written although the reference left it alone")
        else:
            steps = int((g3[h].contiguous().view(torch.int16).int() - w3[h].contiguous().view(torch.int16).int()).abs().max())
            if steps > 1:
                bad.append(f"head {h}: {steps} bf16 steps from the reference")
    return bad


# ----------------------------------------------------------------------------------------------------------------- modules
def rmsnorm(x, scale, exact=False):
    """scale * x / (sqrt(mean(x^2)) + eps): eps is added to the RMS; the normalisation runs in (at least) fp32 and is rounded to x's dtype before
    the scale multiplies it."""
    x, scale = _c(x, exact), _c(scale, exact)
    xf = x if x.dtype in (torch.float32, F64) else x.to(torch.float32)
    norm = xf / (torch.sqrt(torch.mean(xf ** 2, dim=-1, keepdim=True)) + RMS_EPS)
    return scale * norm.to(x.dtype)


def silu(x):
    return x * 1 / (1 + torch.exp(-x))


def attention_core(q, k, v, key_mask=None, scale=None, capture=None):
    """Masked softmax attention on [B, H, S, D] operands as the reference writes it: -inf above the diagonal without a key mask, finfo.min / 2 on
    every hidden pair with one (a fully masked row then attends uniformly)."""
    B, Hq, S, D = q.shape
    rep = Hq // k.shape[1]
    s = (q @ k.repeat_interleave(rep, dim=1).mT) * (D ** -0.5 if scale is None else scale)
    hidden = ~visible(B, S, key_mask)
    if capture is not None:
        capture.append(torch.amax(torch.where(hidden, torch.full((), -torch.inf, dtype=s.dtype), s.detach()), dim=(0, 2, 3)))
    s = s.masked_fill(hidden, -torch.inf if key_mask is None else torch.finfo(s.dtype).min / 2)
    return F.softmax(s, dim=-1) @ v.repeat_interleave(rep, dim=1)


def gqa(sd, pfx, x, cfg, cos, sin, key_mask=None, exact=False, capture=None):
    """GroupedQueryAttention.forward: x [b, s, d_in] -> [b, s, d_out].  ``capture`` (a list) receives the layer's per-head maximum logit."""
    b, s, _ = x.shape
    w = lambda k: _c(sd[pfx + k], exact)
    x = _c(x, exact)
    Hq, Hkv = cfg["n_heads"], cfg["num_kv_groups"]
    D = cfg["emb_dim"] // Hq
    q = F.linear(x, w("w_queries.weight")).view(b, s, Hq, D).transpose(1, 2)
    k = F.linear(x, w("w_keys.weight")).view(b, s, Hkv, D).transpose(1, 2)
    v = F.linear(x, w("w_values.weight")).view(b, s, Hkv, D).transpose(1, 2)
    q, k = rope(q, cos, sin), rope(k, cos, sin)
    o = attention_core(q, k, v, key_mask, capture=capture)
    return F.linear(o.transpose(1, 2).contiguous().view(b, s, Hq * D), w("out_proj.weight"), w("out_proj.bias"))


def block(sd, pfx, x, cfg, cos, sin, key_mask=None, exact=False, capture=None):
    """TransformerBlock.forward on x [b, s, d]."""
    w = lambda k: _c(sd[pfx + k], exact)
    x = _c(x, exact)
    x = gqa(sd, pfx + "att.", rmsnorm(x, w("norm_1.scale"), exact), cfg, cos, sin, key_mask, exact, capture) + x
    h = rmsnorm(x, w("norm_2.scale"), exact)
    x_gate = silu(F.linear(h, w("ffn.lin_gate.weight")))
    return F.linear(F.linear(h, w("ffn.lin1.weight")) * x_gate, w("ffn.lin2.weight")) + x


def tables(cfg):
    return rope_tables(cfg["rope_base"], cfg["emb_dim"] // cfg["n_heads"], cfg["context_length"])


def model(sd, cfg, ids, key_mask=None, exact=False, capture=None):
    """Llama3Model.forward: logits [b, s, vocab]; the head is tied (``emb_dict.weight``)."""
    cos, sin = tables(cfg)
    x = _c(F.embedding(ids, sd["emb_dict.weight"]), exact)
    for i in range(cfg["n_layers"]):
        x = block(sd, f"trf_blocks.{i}.", x, cfg, cos, sin, key_mask, exact, capture)
    return F.linear(rmsnorm(x, _c(sd["final_norm.scale"], exact), exact), _c(sd["emb_dict.weight"], exact))


def model_loss(sd, cfg, ids, targets, key_mask=None, exact=False, capture=None):
    logits = model(sd, cfg, ids, key_mask, exact, capture)
    return F.cross_entropy(logits.flatten(0, 1), targets.flatten()), logits


def model_grads(sd, cfg, ids, targets, key_mask=None, exact=False):
    """-> (loss, logits, {parameter name: gradient}); the tied matrix appears once, as ``emb_dict.weight``."""
    leaves = {k: _c(v, exact).detach().requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and k not in ("out_head.weight", "cos", "sin")}
    loss, logits = model_loss(leaves, cfg, ids, targets, key_mask)
    names = list(leaves)
    grads = torch.autograd.grad(loss, [leaves[n] for n in names])
    return loss.detach(), logits.detach(), dict(zip(names, grads))


# ----------------------------------------------------------------------------------------------------------------- fixtures and operands
def load_fixture(stem="llama3_tiny"):
    """tests/golden/<stem>.safetensors and its .partK continuation files (every committed file stays under 1 MiB) as one dict."""
    from safetensors.torch import load_file

    t = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, stem + ".safetensors")) + glob.glob(os.path.join(GOLDEN, stem + ".part*.safetensors"))):
        t.update(load_file(path))
    if not t:
        raise FileNotFoundError(f"tests/golden/{stem}*.safetensors")
    return t


def state_dict_of(t, prefix="sd."):
    return {k[len(prefix):]: v for k, v in t.items() if k.startswith(prefix)}


def perturb_parameters(named_parameters, gen):
    """The fixture recipe: embedding *= 0.05; every norm scale += 0.1 N(0, 1); out_proj.bias = 0.1 N(0, 1); w_queries and w_keys *= 2 (the logits
    then reach the fixture's threshold), drawn in parameter order from ``gen`` (None: torch's global generator)."""
    with torch.no_grad():
        for k, p in named_parameters:
            if k == "emb_dict.weight":
                p.mul_(0.05)
            elif k.endswith(".scale"):
                p.add_((0.1 * torch.randn(p.shape, generator=gen)).to(p.dtype))
            elif k.endswith("out_proj.bias"):
                p.copy_((0.1 * torch.randn(p.shape, generator=gen)).to(p.dtype))
            elif k.endswith(("w_queries.weight", "w_keys.weight")):
                p.mul_(2)


def attn_operands(B, S, Hq, Hkv, D, seed):
    """q [B, Hq, S, D], k [B, Hkv, S, D] as bf16, N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, Hq, S, D, generator=g).to(BF16), torch.randn(B, Hkv, S, D, generator=g).to(BF16)
