"""Plain-torch restatement of the DeepSeek-V3 dense arithmetic (Multi-head Latent Attention, the block, the MTP module, the main model and the
model loss), written from the formulas of the kernels' contract (include/mi355_vlm.h, csrc/deepseek.hip).  TEST INFRASTRUCTURE ONLY.

Every function runs in one of two flows, chosen by ``dtype``:
  * ``dtype=None``: the reference's dtype flow on the tensors as given -- for bf16 tensors every torch op rounds its result to bf16 where the
    reference's modules do (RMSNorm normalises in fp32, rounds, then multiplies by the scale; the Linears, RoPE, the score matrix, the softmax,
    the weighted sum and SiLU are bf16 ops); for fp32 tensors (the twin's weights) the same ops in fp32;
  * ``dtype=torch.float64``: everything upcast first, no intermediate rounding -- the value every implementation is measured against.
The cos / sin tables are rounded to bf16 first in EVERY flow (``td``): that rounding is part of the function (``RoPE.apply`` casts the tables to
x's dtype, the model's ``.to(bfloat16)`` rounds the buffers themselves, and both fixtures' fp32 twins run on the rounded tables).  Backward functions differentiate the forward ones with autograd.

Attention operands are [B, H, S, D] (the shared rotary key [B, S, Dr]); ``to_tokens`` / ``from_tokens`` convert to the kernels' token-major form.
"""

import glob
import os

import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RMS_EPS = 1e-6
BF16 = torch.bfloat16

TINY_DEEPSEEK = dict(vocab_size=256, context_length=96, emb_dim=64, n_heads=1, n_layers=1, num_ffn=1, hidden_dim=128, mtp_depth=1, mtp_loss_coeff=0.2,
                     rope_base=10000, dtype=torch.bfloat16)
MLA_FIXTURE = dict(d_in=32, d_out=128, num_heads=2, b=2, s=70, context_length=96, rope_base=10000)
# gradients whose floor may exceed 0.1, by name suffix, with the reason (tools/gen_golden_deepseek.py checks the list against the reference's numbers)
FLOOR_ALLOW = {
    ".att.wk_up_proj.bias": "a constant added to every k_nope of a head moves all scores of a query row equally (q . b does not depend on the key), "
                            "so the softmax does not see it: the true gradient is zero and what the reference holds there is rounding noise",
}


def _c(t, dtype):
    return t if dtype is None else t.to(dtype)


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def to_tokens(x):
    """[B, H, S, D] -> [B*S, H*D]"""
    B, H, S, D = x.shape
    return x.transpose(1, 2).reshape(B * S, H * D).contiguous()


def from_tokens(x, B, S, H, D):
    return x.reshape(B, S, H, D).transpose(1, 2)


# ----------------------------------------------------------------------------------------------------------------- pieces
def rope_tables(base, dim, ctx):
    """cos / sin fp32 [ctx, dim]: angle of position m, feature i is m * base^(-2 (i mod dim/2) / dim)."""
    inv = 1.0 / base ** (2 * torch.arange(0, dim // 2, dtype=torch.float32) / dim)
    ang = torch.outer(torch.arange(0, ctx, dtype=torch.float32), inv)
    ang = torch.cat((ang, ang), dim=-1)
    return torch.cos(ang), torch.sin(ang)


def rope(x, cos, sin, table_dtype=None):
    """x [..., S, D]; cos / sin [>= S, D]: cos * x + sin * cat(-x2, x1).  ``table_dtype``: round the tables through it first (bf16 for bf16
    operands -- also in the fp64 flow --, nothing for the fp32 twin)."""
    S, D = x.shape[-2], x.shape[-1]
    c, s = cos[:S], sin[:S]
    if table_dtype is not None:
        c, s = c.to(table_dtype), s.to(table_dtype)
    c, s = c.to(x.dtype), s.to(x.dtype)
    rot = torch.cat((-x[..., D // 2 :], x[..., : D // 2]), dim=-1)
    return c * x + s * rot


def rmsnorm(x, scale, dtype=None):
    """scale * x / (sqrt(mean(x^2)) + eps): eps is added to the RMS; the normalisation runs in (at least) fp32 and is rounded to x's dtype before
    the scale multiplies it."""
    x, scale = _c(x, dtype), _c(scale, dtype)
    xf = x if x.dtype in (torch.float32, torch.float64) else x.to(torch.float32)
    norm = xf / (torch.sqrt(torch.mean(xf ** 2, dim=-1, keepdim=True)) + RMS_EPS)
    return scale * norm.to(x.dtype)


def silu(x):
    return x * 1 / (1 + torch.exp(-x))


def mla_attention(q_nope, q_rope, k_nope, k_rope, v, dtype=None, scale=None):
    """q_nope / k_nope / v [B, H, S, Dn], q_rope [B, H, S, Dr], k_rope [B, S, Dr] (shared by the heads) -> (o [B, H, S, Dn], lse [B, H, S]).
    s = scale * (q_nope . k_nope + q_rope . k_rope) over keys j <= i.  k_rope may also come as [B, H, S, Dr], the shared row already repeated per
    head: a leaf of that shape receives every head's own share of the shared key's gradient (tests/side_attention_sweep.py)."""
    B, H, S, Dn = q_nope.shape
    Dr = q_rope.shape[-1]
    scale = (Dn + Dr) ** -0.5 if scale is None else scale
    q_nope, q_rope, k_nope, k_rope, v = [_c(t, dtype) for t in (q_nope, q_rope, k_nope, k_rope, v)]
    q = torch.cat((q_nope, q_rope), dim=-1)
    k = torch.cat((k_nope, k_rope if k_rope.dim() == 4 else k_rope.unsqueeze(1).expand(-1, H, -1, -1)), dim=-1)
    s = (q @ k.mT) * scale
    s = s.masked_fill(torch.ones(S, S, dtype=torch.bool).triu_(1), -torch.inf)
    p = F.softmax(s, dim=-1)
    return p @ v, torch.logsumexp(s.double() if dtype == torch.float64 else s.float(), dim=-1)


def mla_attention_bwd(q_nope, q_rope, k_nope, k_rope, v, do, dtype=None, scale=None):
    """-> (dq_nope, dq_rope, dk_nope, dk_rope [B, S, Dr] -- summed over heads by the expand's backward --, dv) by autograd."""
    ops = [_c(t, dtype).detach().requires_grad_(True) for t in (q_nope, q_rope, k_nope, k_rope, v)]
    o, _ = mla_attention(*ops, dtype=dtype, scale=scale)
    return torch.autograd.grad(o, ops, _c(do, dtype))


def mla_rope(q_pre, k_pre, cos, sin, dtype=None):
    """q_pre [B, H, S, Dr], k_pre [B, S, Dr] -> rotated, tables rounded to bf16."""
    q_pre, k_pre = _c(q_pre, dtype), _c(k_pre, dtype)
    return rope(q_pre, cos, sin, BF16), rope(k_pre.unsqueeze(1), cos, sin, BF16).squeeze(1)


def mla_rope_bwd(dq, dk_heads, cos, sin, dtype=None):
    """The adjoint rotation of dq [B, H, S, Dr] and of sum_h dk_heads [B, H, S, Dr] -> (dq_pre, dk_pre [B, S, Dr])."""
    q0 = torch.zeros_like(_c(dq, dtype)).requires_grad_(True)
    k0 = torch.zeros_like(_c(dk_heads, dtype)[:, 0]).requires_grad_(True)
    yq, yk = mla_rope(q0, k0, cos, sin, dtype)
    return torch.autograd.grad([yq, yk], [q0, k0], [_c(dq, dtype), _c(dk_heads, dtype).sum(dim=1)])


# ----------------------------------------------------------------------------------------------------------------- modules
def mla(sd, pfx, x, num_heads, cos, sin, dtype=None, capture=None, td=BF16):
    """MultiLatentAttention.forward: x [b, s, d_in] -> [b, s, d_out]."""
    b, s, _ = x.shape
    w = lambda k: _c(sd[pfx + k], dtype)
    lin = lambda t, name: F.linear(t, w(name + ".weight"), w(name + ".bias"))
    x = _c(x, dtype)
    d_out = sd[pfx + "out_proj.weight"].shape[0]
    Dn = d_out // num_heads
    Dr = Dn // 2
    ql = rmsnorm(lin(x, "wq_down_proj"), w("q_rms_norm.scale"), dtype)
    kvl = rmsnorm(lin(x, "wkv_down_proj"), w("kv_rms_norm.scale"), dtype)
    q_nope = lin(ql, "wq_up_proj").view(b, s, num_heads, Dn).transpose(1, 2)
    k_nope = lin(kvl, "wk_up_proj").view(b, s, num_heads, Dn).transpose(1, 2)
    v = lin(kvl, "wv_up_proj").view(b, s, num_heads, Dn).transpose(1, 2)
    q_rope = rope(lin(ql, "wq_decoup").view(b, s, num_heads, Dr).transpose(1, 2), cos, sin, td)
    k_rope = rope(lin(x, "wk_decoup").unsqueeze(1), cos, sin, td).squeeze(1)
    o, _ = mla_attention(q_nope, q_rope, k_nope, k_rope, v)
    if capture is not None:
        capture.update(q=torch.cat((q_nope, q_rope), dim=-1), k=torch.cat((k_nope, k_rope.unsqueeze(1).expand(-1, num_heads, -1, -1)), dim=-1), v=v, ctx=o)
    return lin(o.transpose(1, 2).reshape(b, s, d_out), "out_proj")


def block(sd, pfx, x, cfg, cos, sin, dtype=None, capture=None, td=BF16):
    """TransformerBlock.forward (dense) on x [b, s, d]."""
    w = lambda k: _c(sd[pfx + k], dtype)
    x = _c(x, dtype)
    x = mla(sd, pfx + "att.", rmsnorm(x, w("norm_1.scale"), dtype), cfg["n_heads"], cos, sin, dtype, capture, td) + x
    h = rmsnorm(x, w("norm_2.scale"), dtype)
    return F.linear(F.linear(h, w("ffn.lin1.weight")) * silu(F.linear(h, w("ffn.lin_gate.weight"))), w("ffn.lin2.weight")) + x


def main_model(sd, pfx, cfg, ids, cos, sin, dtype=None, capture=None, td=BF16):
    """MainModel.forward: (logits [b, s, vocab], h_curr [b, s, d])."""
    x = _c(F.embedding(ids, sd[pfx + "emb_layer.weight"]), dtype)
    for i in range(cfg["n_layers"]):
        x = block(sd, f"{pfx}trf_blocks.{i}.", x, cfg, cos, sin, dtype, capture if i == 0 else None, td)
    return F.linear(rmsnorm(x, _c(sd[pfx + "final_norm.scale"], dtype), dtype), _c(sd[pfx + "out_layer.weight"], dtype)), x


def mtp_module(sd, pfx, cfg, ids, h_prev, cos, sin, dtype=None, td=BF16):
    """MTPModule.forward: (logits, h_curr).  The logits come from the down-projected input, not from the block output (as upstream)."""
    w = lambda k: _c(sd[pfx + k], dtype)
    x = rmsnorm(_c(F.embedding(ids, sd[pfx + "emb_layer.weight"]), dtype), w("rms_input.scale"), dtype)
    hp = rmsnorm(_c(h_prev, dtype), w("rms_h_prev.scale"), dtype)
    x = F.linear(torch.cat((x, hp), dim=-1), w("down_proj.weight"), w("down_proj.bias"))
    h_curr = block(sd, pfx + "trf_block.", x, cfg, cos, sin, dtype, None, td)
    return F.linear(x, w("out_layer.weight")), h_curr


def tables(cfg):
    return rope_tables(cfg["rope_base"], cfg["emb_dim"] // cfg["n_heads"] // 2, cfg["context_length"])


def model_loss(sd, cfg, ids, y, shifted_x, shifted_y, dtype=None, capture=None, training=True, td=BF16):
    """DeepSeekV3Model.forward in training mode: (total loss, main logits).  The model's cos / sin are buffers: ``.to(bfloat16)`` rounds them, and
    the fixture's fp32 twin loads the rounded buffers, so every flow of the model sees bf16-rounded tables (``td``)."""
    cos, sin = tables(cfg)
    logits, h_prev = main_model(sd, "main_model.", cfg, ids, cos, sin, dtype, capture, td)
    loss = F.cross_entropy(logits.flatten(0, 1), y.flatten())
    depth = cfg["mtp_depth"]
    if not training or depth == 0:
        return loss, logits
    extra = 0
    for k in range(depth):
        lk, h_prev = mtp_module(sd, f"mtp_modules.{k}.", cfg, shifted_x[k], h_prev, cos, sin, dtype, td)
        extra = extra + F.cross_entropy(lk.flatten(0, 1), shifted_y[k].flatten())
    return loss + (cfg["mtp_loss_coeff"] / depth) * extra, logits


def _shared(k):
    return k.startswith("mtp_modules.") and (".emb_layer." in k or ".out_layer." in k)


def model_grads(sd, cfg, ids, y, shifted_x, shifted_y, dtype=None):
    """-> (loss, logits, {parameter name: gradient}) of the model loss; the shared embedding / head appear once, under their main_model names."""
    td = BF16  # the model's tables are buffers: they are rounded by .to(bfloat16), and the fp32 twin loads those rounded buffers
    leaves = {k: _c(v, dtype).detach().requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and not _shared(k)}
    full = dict(leaves)
    for k in sd:
        if _shared(k):
            full[k] = leaves["main_model." + k.split(".", 2)[2]]
    loss, logits = model_loss(full, cfg, ids, y, shifted_x, shifted_y, td=td)
    names = list(leaves)
    grads = torch.autograd.grad(loss, [leaves[n] for n in names], allow_unused=True)
    return loss.detach(), logits.detach(), {n: (g if g is not None else torch.zeros_like(leaves[n])) for n, g in zip(names, grads)}


def mla_grads(sd, x, dy, num_heads, cos, sin, dtype=None):
    """MultiLatentAttention on its own: -> (y, dx, {parameter name: gradient})."""
    leaves = {k: _c(v, dtype).detach().requires_grad_(True) for k, v in sd.items()}
    xg = _c(x, dtype).detach().requires_grad_(True)
    yv = mla(leaves, "", xg, num_heads, cos, sin)
    names = list(leaves)
    grads = torch.autograd.grad(yv, [xg] + [leaves[n] for n in names], _c(dy, dtype))
    return yv.detach(), grads[0], dict(zip(names, grads[1:]))


# ----------------------------------------------------------------------------------------------------------------- fixtures and operands
def load_fixture(stem="deepseek_tiny"):
    """tests/golden/<stem>.safetensors and its .partK continuation files (every committed file stays under 1 MiB) as one dict."""
    from safetensors.torch import load_file

    t = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, stem + ".safetensors")) + glob.glob(os.path.join(GOLDEN, stem + ".part*.safetensors"))):
        t.update(load_file(path))
    if not t:
        raise FileNotFoundError(f"tests/golden/{stem}*.safetensors")
    return t


def perturb_parameters(named_parameters, gen):
    """The fixture recipe: embedding ~ N(0, 0.05); every norm scale moved off 1 and every bias off its initial value by 0.1 * N(0, 1), drawn in
    parameter order from ``gen``."""
    with torch.no_grad():
        for k, p in named_parameters:
            if k.endswith("emb_layer.weight"):
                p.copy_((torch.randn(p.shape, generator=gen) * 0.05).to(p.dtype))
            elif k.endswith((".scale", ".bias")):
                p.add_((0.1 * torch.randn(p.shape, generator=gen)).to(p.dtype))


def floor_allowed(name):
    return name.endswith(tuple(FLOOR_ALLOW))


def mla_operands(B, S, H, Dn, Dr, seed):
    """q_nope, q_rope, k_nope, k_rope, v, do as bf16, N(0, 1): [B, H, S, D] and the shared key [B, S, Dr]."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *shape: torch.randn(*shape, generator=g).to(BF16)
    return rn(B, H, S, Dn), rn(B, H, S, Dr), rn(B, H, S, Dn), rn(B, S, Dr), rn(B, H, S, Dn), rn(B, H, S, Dn)
