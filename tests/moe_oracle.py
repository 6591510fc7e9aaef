"""Plain-torch restatement of the Qwen3 mixture-of-experts arithmetic: the router, the token-to-expert plan, the layer, the block and the model,
written from the formulas of the kernels' contract (include/mi355_vlm.h, csrc/moe.hip).  TEST INFRASTRUCTURE ONLY.

Every function runs in one of two flows, chosen by ``dtype``:
  * ``dtype=None``: the reference's dtype flow on the tensors as given -- for bf16 tensors every torch op rounds its result to bf16 where the
    reference's modules do (the gate's logits, the softmax, the sum of the selected probabilities, the weights, every expert's output times its
    weight, and the output after EVERY expert's ``index_add_``, experts ascending); for fp32 tensors (the twin's weights) the same ops in fp32;
  * ``dtype=torch.float64``: everything upcast first, no intermediate rounding -- the value every implementation is measured against.
The cos / sin tables are rounded to bf16 first in EVERY flow: the fixture's model is ``.to(bfloat16)`` (which rounds the buffers), and its fp32 twin
loads those buffers.  The top-k selection is explicit: the k largest probabilities in descending order, the lower expert index first among equal
values (``torch.topk`` promises no order there).  Backward functions differentiate the forward ones with autograd; the selection is a constant.
"""

import glob
import os

import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BF16 = torch.bfloat16
RMS_EPS = 1e-6

# the attention dimensions of TINY_QWEN (tests/golden/qwen3_tiny.safetensors), two MoE blocks
TINY_MOE = dict(vocab_size=256, context_length=64, emb_dim=128, n_heads=4, num_kv_groups=2, head_dim=128, n_layers=2, rope_base=1_000_000,
                tie_embeddings=False, model_type="moe", num_experts=8, top_k=2, moe_hidden_dim=32, aux_loss_coef=0.001, dtype=torch.bfloat16)
FIXTURE_BATCH, FIXTURE_SEQ = 2, 48
# gradients whose floor may exceed 0.1, by name suffix, with the reason (tools/gen_golden_moe.py checks the list against the reference's numbers)
FLOOR_ALLOW = {}


def floor_allowed(name):
    return any(name.endswith(s) for s in FLOOR_ALLOW)


def _c(t, dtype):
    return t if dtype is None else t.to(dtype)


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ----------------------------------------------------------------------------------------------------------------- router and plan
def topk_lowest_index_first(p, k):
    """(values, indices) of the k largest entries of every row, descending; among equal values the lower index first (a stable sort)."""
    v, i = torch.sort(p, dim=-1, descending=True, stable=True)
    return v[:, :k], i[:, :k]


def boundary_tie(p, k):
    """Rows whose k-th and (k+1)-th largest values are equal: the selected SET then depends on the tie rule.  [T] bool; all False at k == E."""
    if k >= p.shape[1]:
        return torch.zeros(p.shape[0], dtype=torch.bool)
    v, _ = torch.sort(p, dim=-1, descending=True, stable=True)
    return v[:, k - 1] == v[:, k]


def route(gate_in, k, replay=False, dtype=None, idx=None):
    """-> (p [T, E], idx int64 [T, k], w [T, k], s [T]).  ``gate_in``: logits, or with ``replay`` the probabilities.  ``idx``: a selection to
    use instead of this flow's own (the fp64 flow judged per slot against a bf16 selection)."""
    x = _c(gate_in, dtype)
    p = x if replay else F.softmax(x, dim=-1)
    if idx is None:
        v, idx = topk_lowest_index_first(p, k)
    else:
        v = p.gather(1, idx)
    s = v.sum(dim=-1, keepdim=True)
    return p, idx, v / s, s.squeeze(-1)


def load_loss(p, idx, coef):
    """qwen3_moe.py:124-129: coef * E * <f, P>, f = counts / (k T) in p's dtype (no gradient), P = mean_t p."""
    T, E = p.shape
    counts = torch.bincount(idx.reshape(-1), minlength=E).to(p.dtype)
    f = counts / (idx.shape[1] * T)
    return coef * (E * torch.dot(f, p.mean(dim=0)))


def route_bwd(gate_in, k, dw, g, coef, dtype=None, idx=None):
    """d(logits) for the upstream gradient ``dw`` [T, k] of the weights and ``g`` of the load loss (a float), by autograd."""
    x = _c(gate_in, dtype).detach().requires_grad_(True)
    p, idx, w, _ = route(x, k, dtype=dtype, idx=idx)
    total = (w * _c(dw, w.dtype)).sum() + g * load_loss(p, idx, coef)
    return torch.autograd.grad(total, x)[0]


def plan(idx, E, align):
    """The expert-sorted layout: (counts [E], offsets [E + 1], slot [T, k], row_token [R]), R = T k + E (align - 1); int64."""
    T, k = idx.shape
    flat = idx.reshape(-1)
    counts = torch.bincount(flat, minlength=E)
    padded = (counts + align - 1) // align * align
    offsets = torch.cat([torch.zeros(1, dtype=torch.long), padded.cumsum(0)])
    order = torch.sort(flat, stable=True)[1]  # assignments (t, j) ascending inside an expert
    rank = torch.arange(T * k) - (counts.cumsum(0) - counts)[flat[order]]
    slot = torch.empty(T * k, dtype=torch.long)
    slot[order] = offsets[flat[order]] + rank
    row_token = torch.full((T * k + E * (align - 1),), -1, dtype=torch.long)
    row_token[slot] = torch.arange(T * k) // k
    return counts, offsets, slot.view(T, k), row_token


# ----------------------------------------------------------------------------------------------------------------- the layer
def expert(x, w1, wg, w2):
    """Expert.forward (qwen3_moe.py:61-66): lin2(lin1(x) * silu(lin_gate(x)))."""
    return F.linear(F.linear(x, w1) * F.silu(F.linear(x, wg)), w2)


def moe_layer(sd, pfx, x2d, cfg, gate_probas=None, training=True, dtype=None):
    """Qwen3MoE.forward on [T, d] (qwen3_moe.py:104-167) -> (out [T, d], p [T, E], load loss or None, idx [T, k])."""
    E, k = cfg["num_experts"], cfg["top_k"]
    x = _c(x2d, dtype)
    g = lambda name: _c(sd[pfx + name], dtype)
    if gate_probas is None:
        p, idx, w, _ = route(F.linear(x, g("gate.weight")), k)
    else:
        p, idx, w, _ = route(gate_probas.detach().to(x.dtype), k, replay=True)
    loss = load_loss(p, idx, cfg["aux_loss_coef"]) if training else None
    out = torch.zeros_like(x)
    for e in range(E):
        tok, pos = torch.where(idx == e)
        if tok.numel() == 0:
            continue
        y = expert(x[tok], g(f"experts.{e}.lin1.weight"), g(f"experts.{e}.lin_gate.weight"), g(f"experts.{e}.lin2.weight"))
        out = out.index_add(0, tok, y * w[tok, pos].unsqueeze(-1))
    return out, p, loss, idx


# ----------------------------------------------------------------------------------------------------------------- block and model
def rmsnorm(x, weight, dtype=None):
    """PytorchRMSNorm: x * rsqrt(mean(x^2) + eps) * w in (at least) fp32, rounded to x's dtype."""
    x, weight = _c(x, dtype), _c(weight, dtype)
    up = x.dtype if x.dtype == torch.float64 else torch.float32
    xf = x.to(up)
    return (xf * torch.rsqrt(xf.pow(2).mean(dim=-1, keepdim=True) + RMS_EPS) * weight.to(up)).to(x.dtype)


def rope_tables(cfg):
    """cos / sin [ctx, head_dim], fp32 values rounded through bf16 (see the module docstring)."""
    dim = cfg["head_dim"]
    inv = 1.0 / cfg["rope_base"] ** (2 * torch.arange(0, dim // 2, dtype=torch.float32) / dim)
    ang = torch.outer(torch.arange(0, cfg["context_length"], dtype=torch.float32), inv)
    ang = torch.cat((ang, ang), dim=-1)
    return torch.cos(ang).to(BF16).float(), torch.sin(ang).to(BF16).float()


def rope(x, cos, sin):
    S, D = x.shape[-2], x.shape[-1]
    c, s = cos[:S].to(x.dtype), sin[:S].to(x.dtype)
    return c * x + s * torch.cat((-x[..., D // 2 :], x[..., : D // 2]), dim=-1)


def attention(sd, pfx, x, cfg, cos, sin, dtype=None):
    """GroupedQueryAttention.forward (qwen3_attention.py:81-150): QK-norm before RoPE, causal, masked scores filled with finfo.min / 2."""
    b, s, _ = x.shape
    hq, hkv, dh = cfg["n_heads"], cfg["num_kv_groups"], cfg["head_dim"]
    g = lambda name: _c(sd[pfx + name], dtype)
    heads = lambda t, h: t.view(b, s, h, dh).transpose(1, 2)
    q, k, v = heads(F.linear(x, g("w_queries.weight")), hq), heads(F.linear(x, g("w_keys.weight")), hkv), heads(F.linear(x, g("w_values.weight")), hkv)
    q, k = rope(rmsnorm(q, g("q_norm.weight")), cos, sin), rope(rmsnorm(k, g("k_norm.weight")), cos, sin)
    src = torch.arange(hq) // (hq // hkv)
    scores = (q @ k[:, src].mT) * dh ** -0.5
    scores = scores.masked_fill(torch.ones(s, s, dtype=torch.bool).triu_(1), torch.finfo(scores.dtype).min / 2)
    ctx = (F.softmax(scores, dim=-1) @ v[:, src]).transpose(1, 2).reshape(b, s, hq * dh)
    return F.linear(ctx, g("out_proj.weight"))


def block(sd, pfx, x, cfg, cos, sin, gate_probas=None, training=True, dtype=None):
    """MoETransformerBlock.forward (qwen3_transformer_block.py:126-153) -> (x, p, load loss, idx)."""
    x = _c(x, dtype)
    x = attention(sd, pfx + "att.", rmsnorm(x, sd[pfx + "norm1.weight"], dtype), cfg, cos, sin, dtype) + x
    h = rmsnorm(x, sd[pfx + "norm2.weight"], dtype)
    out, p, loss, idx = moe_layer(sd, pfx + "moe.", h.reshape(-1, h.shape[-1]), cfg, gate_probas, training, dtype)
    return out.view_as(x) + x, p, loss, idx


def model(sd, cfg, ids, gate_probas=None, training=True, dtype=None):
    """Qwen3MoEModel.forward -> (logits, [p per layer], [load loss per layer], [idx per layer])."""
    cos, sin = rope_tables(cfg)
    x = F.embedding(ids, _c(sd["emb_dict.weight"], dtype))
    ps, losses, idxs = [], [], []
    for i in range(cfg["n_layers"]):
        gp = gate_probas[i] if isinstance(gate_probas, (list, tuple)) else gate_probas
        x, p, loss, idx = block(sd, f"trf_blocks.{i}.", x, cfg, cos, sin, gp, training, dtype)
        ps.append(p)
        losses.append(loss)
        idxs.append(idx)
    return F.linear(rmsnorm(x, sd["final_norm.weight"], dtype), _c(sd["out_head.weight"], dtype)), ps, losses, idxs


def model_loss(sd, cfg, ids, targets, gate_probas=None, dtype=None):
    """The fixture's loss: CE (ignore_index -100) plus every layer's load loss, added by hand.  -> (loss, logits, [p per layer])."""
    logits, ps, losses, _ = model(sd, cfg, ids, gate_probas, True, dtype)
    loss = F.cross_entropy(logits.flatten(0, 1), targets.flatten())
    for l in losses:
        loss = loss + l
    return loss, logits, ps


def model_grads(sd, cfg, ids, targets, gate_probas=None, dtype=None):
    """-> (loss, logits, {name: gradient}) by autograd over the floating-point entries of ``sd``."""
    leaves = {k: _c(v, dtype).detach().requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and k not in ("cos", "sin")}
    loss, logits, _ = model_loss({**sd, **leaves}, cfg, ids, targets, gate_probas, None)
    names = list(leaves)
    grads = torch.autograd.grad(loss, [leaves[n] for n in names], allow_unused=True)
    return loss.detach(), logits.detach(), {n: (torch.zeros_like(leaves[n]) if g is None else g) for n, g in zip(names, grads)}


# ----------------------------------------------------------------------------------------------------------------- fixture and operands
def load_fixture(stem="moe_tiny"):
    """tests/golden/<stem>.safetensors and its .partK continuation files (every committed file stays under 1 MiB) as one dict."""
    from safetensors.torch import load_file

    t = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, stem + ".safetensors")) + glob.glob(os.path.join(GOLDEN, stem + ".part*.safetensors"))):
        t.update(load_file(path))
    if not t:
        raise FileNotFoundError(f"tests/golden/{stem}*.safetensors")
    return t


def perturb_parameters(named_parameters, gen=None):
    """Move the norm weights off 1 and sharpen the gate (fresh gate weights give near-uniform probabilities, where every token sits on a near-tie):
    norm weights += 0.1 N(0, 1), gate weights *= 8, drawn in parameter order from ``gen``.  Used by the fixture generator."""
    with torch.no_grad():
        for k, p in named_parameters:
            if k.endswith("norm.weight") or k.endswith("norm1.weight") or k.endswith("norm2.weight"):
                p.add_((0.1 * torch.randn(p.shape, generator=gen)).to(p.dtype))
            elif k.endswith("moe.gate.weight"):
                p.mul_(8.0)


def logits_without_boundary_tie(T, E, k, seed, std=2.0):
    """bf16 logits [T, E] ~ N(0, std), every row redrawn until its bf16 probabilities have no tie at the k-th / (k+1)-th place."""
    g = torch.Generator().manual_seed(seed)
    x = (std * torch.randn(T, E, generator=g)).to(BF16)
    for _ in range(64):
        bad = boundary_tie(F.softmax(x, dim=-1), k)
        if not bool(bad.any()):
            return x
        x[bad] = (std * torch.randn(int(bad.sum()), E, generator=g)).to(BF16)
    raise RuntimeError("could not draw tie-free logits")
