"""Plain-torch restatement of the classic-MoE arithmetic: the softmax router with its load and z losses, the experts' bias + GELU, an expert and the
layer, written from the formulas of the kernels' contract (include/mi355_vlm.h, csrc/classic_moe.hip).  TEST INFRASTRUCTURE ONLY.

Every function runs in one of two flows, chosen by ``dtype`` (as tests/deepseek_moe_oracle.py and tests/latent_moe_oracle.py, whose helpers are imported,
not copied):
  * ``dtype=None``: the reference's dtype flow on the tensors as given -- for bf16 tensors every torch op rounds its result to bf16 where the
    reference's modules do: the gate's addmm, the softmax, the sum of the selected probabilities and the division by it; ``logsumexp``, its square and
    the mean over the tokens; the counts CAST TO THE ACTIVATION DTYPE before f = counts / (k T), the mean of the probabilities, the dot product and every
    product and sum of the loss; an expert's two addmm and every elementwise step of the GELU (x * 0.5, x / sqrt 2, erf, 1 + erf, the product); every
    expert's output times its weight and the output after EVERY hit expert's ``index_add_``, experts ascending; for fp32 tensors the same ops in fp32;
  * ``dtype=torch.float64``: everything upcast first, no intermediate rounding -- the value every implementation is measured against.
The top-k selection is explicit: the k largest probabilities in descending order, the lower expert index first among equal values.  The selection is a
constant of the backward, and so is f.  Where a selection enters, ``idx`` gives one to evaluate on.
"""

import math

import torch
import torch.nn.functional as F

from deepseek_moe_oracle import GOLDEN, _c, boundary_tie, counts_of, load_fixture, logits_without_boundary_tie, rel_l2, topk_lowest_index_first  # noqa: F401

BF16 = torch.bfloat16

# the two fixture layers (tools/gen_golden_classic_moe.py), input (2, 35, emb_dim)
FIXTURE_LAYERS = {
    "A": dict(cfg=dict(emb_dim=80), kwargs=dict(num_experts=3, top_k=1, scaling_factor=0.125), E=3, k=1, hidden=40),  # hidden no multiple of 32, padded gate
    "B": dict(cfg=dict(emb_dim=64), kwargs=dict(), E=8, k=2, hidden=128),  # the upstream defaults: 8 experts, top-2, "auto"
}
FIXTURE_BATCH, FIXTURE_SEQ = 2, 35
LOAD_COEFF, Z_COEFF = 10e-2, 1e-3


def tie_free_logits(T, E, k, seed, std=2.0):
    """bf16 logits [T, E] without a boundary tie in the bf16 probabilities (the shared generator with balancing biases of zero)."""
    return logits_without_boundary_tie(T, E, k, torch.zeros(E, dtype=BF16), seed, std)


# ----------------------------------------------------------------------------------------------------------------- router and loss
def route(logits, k, dtype=None, idx=None):
    """-> (p [T, E], idx int64 [T, k], w [T, k], s [T], lse [T]) (classic_moe.py:84-89).  ``idx``: a selection to use instead of this flow's own; an entry
    that is no expert weighs 0."""
    x = _c(logits, dtype)
    E = x.shape[1]
    p = F.softmax(x, dim=-1)
    if idx is None:
        _, idx = topk_lowest_index_first(p, k)
    ok = (idx >= 0) & (idx < E)
    v = torch.where(ok, p.gather(1, idx.clamp(0, E - 1)), torch.zeros((), dtype=p.dtype))
    s = v.sum(dim=-1, keepdim=True)
    return p, idx, v / s, s.squeeze(-1), torch.logsumexp(x, dim=-1)


def moe_loss(p, idx, lse, load_coeff=LOAD_COEFF, z_coeff=Z_COEFF):
    """classic_moe.py:89-96: z_coeff * mean(lse^2) + load_coeff * E * <f, P>, f = counts.to(p.dtype) / (k T) (no gradient), P = mean_t p."""
    T, E = p.shape
    z = (lse ** 2).mean()
    sel = idx.reshape(-1)
    counts = torch.bincount(sel[(sel >= 0) & (sel < E)], minlength=E).to(dtype=p.dtype)
    f = counts / (idx.shape[1] * T)
    load = E * torch.dot(f, torch.mean(p, dim=0))
    return z_coeff * z + load_coeff * load


def route_bwd(logits, k, dw, g, load_coeff=LOAD_COEFF, z_coeff=Z_COEFF, dtype=None, idx=None):
    """d(logits) for the upstream gradient ``dw`` [T, k] of the weights and ``g`` (a float, or None: no loss term) of moe_loss, by autograd."""
    x = _c(logits, dtype).detach().requires_grad_(True)
    p, idx, w, _, lse = route(x, k, idx=idx)
    total = (w * _c(dw, w.dtype)).sum()
    if g is not None:
        total = total + g * moe_loss(p, idx, lse, load_coeff, z_coeff)
    return torch.autograd.grad(total, x)[0]


# ----------------------------------------------------------------------------------------------------------------- bias, activation, expert
def gelu(x):
    """The reference's GELU module: x * 1/2 * (1 + erf(x / sqrt 2)), step by step in x's dtype."""
    return x * 0.5 * (1 + torch.erf(x / math.sqrt(2)))


def row_experts(counts, offsets, R):
    """[R] int64: the expert whose segment holds the sorted row, -1 on padding rows."""
    e_of = torch.full((R,), -1, dtype=torch.long)
    for e, (c, o) in enumerate(zip(counts.tolist(), offsets.tolist())):
        e_of[o : o + c] = e
    return e_of


def bias_act_grads(z, bias, e_of, dact, dtype=None):
    """On the rows with an expert (the others are returned as zeros): -> (pre = z + bias[e], act = gelu(pre), dpre for the upstream ``dact``)."""
    zz = _c(z, dtype)
    live = e_of >= 0
    pre = torch.zeros_like(zz)
    pre[live] = zz[live] + _c(bias, dtype)[e_of[live]]
    pre = pre.detach().requires_grad_(True)
    act = gelu(pre)
    dpre = torch.autograd.grad(act, pre, _c(dact, dtype))[0]
    keep = live.unsqueeze(1)
    return pre.detach() * keep, act.detach() * keep, dpre * keep


def segment_colsum(x, counts, offsets, dtype=torch.float64):
    """[E, N]: the column sums over every expert's segment."""
    xx = x.to(dtype)
    return torch.stack([xx[o : o + c].sum(dim=0) for c, o in zip(counts.tolist(), offsets.tolist())])


def expert(x, w1, b1, w2, b2):
    """ExpertGeLU.forward (classic_moe.py:23-30)."""
    return F.linear(gelu(F.linear(x, w1, b1)), w2, b2)


def expert_grads(x, w1, b1, w2, b2, dy, dtype=None):
    """-> (y, dx, d w1, d b1, d w2, d b2)."""
    ops = [_c(t, dtype).detach().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    y = expert(*ops)
    return (y.detach(),) + tuple(torch.autograd.grad(y, ops, _c(dy, dtype)))


# ----------------------------------------------------------------------------------------------------------------- the layer
def layer(sd, x2d, k, load_coeff=LOAD_COEFF, z_coeff=Z_COEFF, dtype=None, idx=None, record=None):
    """MoE.forward on [T, d] -> (out [T, d], moe_loss, idx [T, k]).  The dispatch is upstream's: the hit experts ascending, one ``index_add_`` each."""
    E = sd["gate.weight"].shape[0]
    x = _c(x2d, dtype)
    g = lambda name: _c(sd[name], dtype)
    logits = F.linear(x, g("gate.weight"), g("gate.bias"))
    p, idx, w, _, lse = route(logits, k, idx=idx)
    loss = moe_loss(p, idx, lse, load_coeff, z_coeff)
    out = torch.zeros_like(x)
    for e in range(E):
        tok, pos = torch.where(idx == e)
        if tok.numel() == 0:
            continue
        pre = f"experts.{e}.layers."
        y = expert(x[tok], g(pre + "0.weight"), g(pre + "0.bias"), g(pre + "2.weight"), g(pre + "2.bias"))
        out = out.index_add(0, tok, y * w[tok, pos].unsqueeze(-1))
    if record is not None:
        record.update(out=out.detach(), loss=loss.detach(), logits=logits.detach(), p=p.detach(), idx=idx, w=w.detach(), counts=counts_of(idx, E))
    return out, loss, idx


def layer_grads(sd, x2d, k, dy, g_loss, load_coeff=LOAD_COEFF, z_coeff=Z_COEFF, dtype=None, idx=None):
    """-> (out, moe_loss, dx, {name: gradient}, idx) under the total (out * dy).sum() + g_loss * moe_loss; an expert without a token has a zero gradient."""
    leaves = {n: _c(v, dtype).detach().requires_grad_(True) for n, v in sd.items()}
    xg = _c(x2d, dtype).detach().requires_grad_(True)
    out, loss, idx = layer(leaves, xg, k, load_coeff, z_coeff, idx=idx)
    names = list(leaves)
    total = (out * _c(dy, out.dtype)).sum() + g_loss * loss
    grads = torch.autograd.grad(total, [xg] + [leaves[n] for n in names], allow_unused=True)
    return out.detach(), loss.detach(), grads[0], {n: (torch.zeros_like(leaves[n]) if g is None else g) for n, g in zip(names, grads[1:])}, idx
