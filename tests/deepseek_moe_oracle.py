"""Plain-torch restatement of the DeepSeekMoE arithmetic: the bias-balanced router, the bias update, the shared experts, the layer, the block and
the model with MoE blocks, written from the formulas of the kernels' contract (include/mi355_vlm.h, csrc/deepseek_moe.hip).  TEST INFRASTRUCTURE
ONLY.  Attention, norms and the MTP modules are tests/deepseek_oracle.py's.

Every function runs in one of two flows, chosen by ``dtype``:
  * ``dtype=None``: the reference's dtype flow on the tensors as given -- for bf16 tensors every torch op rounds its result to bf16 where the
    reference's modules do (the gate's addmm, the softmax, the biased key in the promoted dtype of p and the buffer, the sum of the selected
    probabilities, the weights; the shared experts' matmul, bias add, SiLU, second matmul, bias add and the sum over the experts; every routed
    expert's output times its weight and the output after EVERY expert's ``index_add_``, experts ascending); for fp32 tensors the same ops in fp32;
  * ``dtype=torch.float64``: everything upcast first, no intermediate rounding -- the value every implementation is measured against.
The top-k selection is explicit: the k largest keys in descending order, the lower expert index first among equal keys (``torch.topk`` promises no
order there).  The selection is a constant of the backward; ``biases`` carries no gradient.
"""

import torch
import torch.nn.functional as F

import deepseek_oracle as DO
from deepseek_oracle import GOLDEN, _c, load_fixture, rel_l2  # noqa: F401
from moe_oracle import boundary_tie, topk_lowest_index_first

BF16 = torch.bfloat16

# TINY_DEEPSEEK's dimensions, three blocks of which two hold a DeepSeekMoE (7 routed + 1 shared expert, hidden 128 / 4 = 32)
TINY_DEEPSEEK_MOE = dict(DO.TINY_DEEPSEEK, n_layers=3, num_ffn=1, num_experts=8, num_shared_experts=1, top_k=3, moe_scaling_factor="auto",
                         moe_bias_update_rate=1e-3)
FIXTURE_BATCH, FIXTURE_SEQ = 2, 70
# gradients whose floor may exceed 0.1, by name suffix, with the reason (tools/gen_golden_deepseek_moe.py checks the list against the reference)
FLOOR_ALLOW = dict(DO.FLOOR_ALLOW)


def floor_allowed(name):
    return name.endswith(tuple(FLOOR_ALLOW))


def moe_layers(cfg):
    return list(range(cfg["num_ffn"], cfg["n_layers"]))


# ----------------------------------------------------------------------------------------------------------------- router
def biased_key(p, biases):
    """p + biases as torch computes it: in the promoted dtype of the two (bf16 + bf16 -> a bf16 sum, bf16 + fp32 -> fp32)."""
    return p + biases


def route(logits, biases, k, dtype=None, idx=None):
    """-> (p [T, E], idx int64 [T, k], w [T, k], s [T]).  ``idx``: a selection to use instead of this flow's own."""
    x = _c(logits, dtype)
    p = F.softmax(x, dim=-1)
    if idx is None:
        _, idx = topk_lowest_index_first(biased_key(p, _c(biases, dtype)), k)
    v = p.gather(1, idx)
    s = v.sum(dim=-1, keepdim=True)
    return p, idx, v / s, s.squeeze(-1)


def route_bwd(logits, biases, k, dw, dtype=None, idx=None):
    x = _c(logits, dtype).detach().requires_grad_(True)
    _, _, w, _ = route(x, biases, k, dtype=dtype, idx=idx)
    return torch.autograd.grad((w * _c(dw, w.dtype)).sum(), x)[0]


def key_boundary_tie(logits, biases, k):
    """Rows whose k-th and (k+1)-th largest BIASED keys are equal (reference dtype flow)."""
    return boundary_tie(biased_key(F.softmax(logits, dim=-1), biases), k)


def logits_without_boundary_tie(T, E, k, biases, seed, std=2.0):
    """bf16 logits [T, E] ~ N(0, std), every row redrawn until its biased keys have no tie at the k-th / (k+1)-th place."""
    g = torch.Generator().manual_seed(seed)
    x = (std * torch.randn(T, E, generator=g)).to(BF16)
    for _ in range(64):
        bad = key_boundary_tie(x, biases, k)
        if not bool(bad.any()):
            return x
        x[bad] = (std * torch.randn(int(bad.sum()), E, generator=g)).to(BF16)
    raise RuntimeError("could not draw tie-free logits")


def robust_tokens(logits, biases, k):
    """[T] bool: the selected SET survives every move of the bf16 logits by one bf16 ulp each in the worst direction -- the selected experts' logits
    one ulp down and all others one ulp up, and the reverse for the softmax's normalisation -- judged on the keys of the reference dtype flow."""
    def ulp_move(x, up):
        bits = x.view(torch.int16).to(torch.int32)
        step = torch.where((x >= 0) == up, 1, -1)
        zero = x == 0
        moved = (bits + step).to(torch.int16).view(BF16)
        tiny = torch.tensor(2.0 ** -133, dtype=torch.float32).to(BF16)
        return torch.where(zero, tiny if up else -tiny, moved)

    E = logits.shape[1]
    _, idx0 = topk_lowest_index_first(biased_key(F.softmax(logits, dim=-1), biases), k)
    sel = torch.zeros_like(logits, dtype=torch.bool).scatter_(1, idx0, True)
    ok = torch.ones(logits.shape[0], dtype=torch.bool)
    if k >= E:
        return ok
    worst = torch.where(sel, ulp_move(logits, False), ulp_move(logits, True))
    key = biased_key(F.softmax(worst, dim=-1), biases).float()
    lo_sel = key.masked_fill(~sel, float("inf")).min(dim=1).values
    hi_rest = key.masked_fill(sel, float("-inf")).max(dim=1).values
    return ok & (lo_sel > hi_rest)


# ----------------------------------------------------------------------------------------------------------------- bias update
def counts_of(idx, E):
    return torch.bincount(idx.reshape(-1), minlength=E)


def max_violation(counts, dtype=None):
    c = counts.float() if dtype is None else counts.to(dtype)
    mean = c.mean()
    return (c.max() - mean) / mean


def bias_update(biases, counts, rate):
    """deepseek_moe.py:208-210 on a copy: the increment is an fp32 tensor, the in-place add rounds to the buffer's dtype."""
    c = counts.float()
    b = biases.clone()
    b += rate * (c.mean() - c).sign()
    return b


# ----------------------------------------------------------------------------------------------------------------- experts
def shared_experts(x2d, w1, b1, w2, b2, dtype=None):
    """VectorizedSharedExperts.forward on [T, d]: w1 [n, d, h], b1 [n, h], w2 [n, h, d], b2 [n, d]."""
    x, w1, b1, w2, b2 = [_c(t, dtype) for t in (x2d, w1, b1, w2, b2)]
    h = x.unsqueeze(0) @ w1  # [n, T, h]
    h = h + b1.unsqueeze(1)
    h = F.silu(h)
    y = h @ w2
    y = y + b2.unsqueeze(1)
    return torch.sum(y, dim=0)


def shared_grads(x2d, w1, b1, w2, b2, dy, dtype=None):
    ops = [_c(t, dtype).detach().requires_grad_(True) for t in (x2d, w1, b1, w2, b2)]
    y = shared_experts(*ops)
    return (y.detach(),) + tuple(torch.autograd.grad(y, ops, _c(dy, dtype)))


def expert(x, w1, wg, w2):
    """Expert.forward (deepseek_moe.py:30-35): lin2(silu(lin1(x)) * lin_gate(x))."""
    return F.linear(F.silu(F.linear(x, w1)) * F.linear(x, wg), w2)


def moe_layer(sd, pfx, x2d, cfg, dtype=None, idx=None, record=None):
    """DeepSeekMoE.forward on [T, d] with the buffer ``sd[pfx + 'biases']`` as it stands BEFORE the forward -> (out [T, d], idx [T, k]).
    ``record`` (a dict) receives logits, p, idx, w, counts, the updated biases and max_vio."""
    E = cfg["num_experts"] - cfg["num_shared_experts"]
    k = cfg["top_k"]
    x = _c(x2d, dtype)
    g = lambda name: _c(sd[pfx + name], dtype)
    out = torch.zeros_like(x)
    if cfg["num_shared_experts"] > 0:
        out = out + shared_experts(x, g("shared_experts.lin1.weight"), g("shared_experts.lin1.bias"), g("shared_experts.lin2.weight"), g("shared_experts.lin2.bias"))
    logits = F.linear(x, g("gate.weight"), g("gate.bias"))
    biases = sd[pfx + "biases"].detach()
    p, idx, w, _ = route(logits, biases, k, idx=idx)
    for e in range(E):
        tok, pos = torch.where(idx == e)
        if tok.numel() == 0:
            continue
        y = expert(x[tok], g(f"routed_experts.{e}.lin1.weight"), g(f"routed_experts.{e}.lin_gate.weight"), g(f"routed_experts.{e}.lin2.weight"))
        out = out.index_add(0, tok, y * w[tok, pos].unsqueeze(-1))
    if record is not None:
        counts = counts_of(idx, E)
        record.update(x=x2d.detach(), out=out.detach(), logits=logits.detach(), p=p.detach(), idx=idx, w=w.detach(), counts=counts,
                      biases=bias_update(biases, counts, cfg["moe_bias_update_rate"]), max_vio=max_violation(counts, dtype))
    return out, idx


def layer_grads(sd, pfx, x2d, cfg, dy, dtype=None, idx=None):
    """-> (out, dx, {name: gradient}, idx) of the layer on its own; an expert without a token has a zero gradient."""
    leaves = {n: _c(v, dtype).detach().requires_grad_(True) for n, v in sd.items() if n.startswith(pfx) and not n.endswith("biases")}
    xg = _c(x2d, dtype).detach().requires_grad_(True)
    out, idx = moe_layer({**sd, **leaves}, pfx, xg, cfg, idx=idx)
    names = list(leaves)
    grads = torch.autograd.grad(out, [xg] + [leaves[n] for n in names], _c(dy, dtype), allow_unused=True)
    return out.detach(), grads[0], {n: (torch.zeros_like(leaves[n]) if g is None else g) for n, g in zip(names, grads[1:])}, idx


# ----------------------------------------------------------------------------------------------------------------- block and model
def block(sd, pfx, x, cfg, cos, sin, layer, dtype=None, idx=None, record=None, td=BF16):
    """TransformerBlock.forward on x [b, s, d]: the dense block for layer < num_ffn, else MLA + DeepSeekMoE."""
    if layer < cfg["num_ffn"]:
        return DO.block(sd, pfx, x, cfg, cos, sin, dtype, None, td)
    w = lambda name: _c(sd[pfx + name], dtype)
    x = _c(x, dtype)
    x = DO.mla(sd, pfx + "att.", DO.rmsnorm(x, w("norm_1.scale"), dtype), cfg["n_heads"], cos, sin, dtype, None, td) + x
    h = DO.rmsnorm(x, w("norm_2.scale"), dtype)
    out, _ = moe_layer(sd, pfx + "ffn.", h.reshape(-1, h.shape[-1]), cfg, dtype, idx, record)
    return out.view_as(x) + x


def model_loss(sd, cfg, ids, y, shifted_x, shifted_y, dtype=None, idxs=None, records=None, td=BF16):
    """DeepSeekV3Model.forward in training mode with MoE blocks in the main model: (total loss, main logits).  ``idxs`` / ``records``: per MoE layer
    (keyed by the layer number) a forced selection / a dict to fill."""
    cos, sin = DO.tables(cfg)
    pfx = "main_model."
    x = _c(F.embedding(ids, sd[pfx + "emb_layer.weight"]), dtype)
    for i in range(cfg["n_layers"]):
        x = block(sd, f"{pfx}trf_blocks.{i}.", x, cfg, cos, sin, i, dtype, None if idxs is None else idxs.get(i), None if records is None else records.setdefault(i, {}), td)
    logits = F.linear(DO.rmsnorm(x, _c(sd[pfx + "final_norm.scale"], dtype), dtype), _c(sd[pfx + "out_layer.weight"], dtype))
    loss = F.cross_entropy(logits.flatten(0, 1), y.flatten())
    depth = cfg["mtp_depth"]
    h_prev, extra = x, 0
    for k in range(depth):
        lk, h_prev = DO.mtp_module(sd, f"mtp_modules.{k}.", cfg, shifted_x[k], h_prev, cos, sin, dtype, td)
        extra = extra + F.cross_entropy(lk.flatten(0, 1), shifted_y[k].flatten())
    return (loss + (cfg["mtp_loss_coeff"] / depth) * extra if depth else loss), logits


def model_grads(sd, cfg, ids, y, shifted_x, shifted_y, dtype=None, idxs=None, records=None):
    """-> (loss, logits, {parameter name: gradient}); buffers (biases, cos, sin, mask) are constants; the shared embedding / head appear once."""
    is_buf = lambda k: k.endswith(".biases") or k in ("mask", "cos", "sin")
    leaves = {k: _c(v, dtype).detach().requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and not DO._shared(k) and not is_buf(k)}
    full = {**sd, **leaves}
    for k in sd:
        if DO._shared(k):
            full[k] = leaves["main_model." + k.split(".", 2)[2]]
    loss, logits = model_loss(full, cfg, ids, y, shifted_x, shifted_y, idxs=idxs, records=records)
    names = list(leaves)
    grads = torch.autograd.grad(loss, [leaves[n] for n in names], allow_unused=True)
    return loss.detach(), logits.detach(), {n: (g if g is not None else torch.zeros_like(leaves[n])) for n, g in zip(names, grads)}


def layer_state(cfg, seed, biases=None, dtype=BF16):
    """A DeepSeekMoE layer's state_dict drawn from N(0, 1) scaled like the default initialisation, gate sharpened; keys as upstream's."""
    g = torch.Generator().manual_seed(seed)
    d = cfg["emb_dim"]
    ns, E = cfg["num_shared_experts"], cfg["num_experts"] - cfg["num_shared_experts"]
    f = cfg["moe_scaling_factor"]
    f = 1 / (cfg["top_k"] + ns) if f == "auto" else f
    h = int(f * cfg["hidden_dim"])
    r = lambda *shape, scale=1.0: (scale * torch.randn(*shape, generator=g)).to(dtype)
    sd = {}
    for e in range(E):
        sd[f"routed_experts.{e}.lin1.weight"] = r(h, d, scale=d ** -0.5)
        sd[f"routed_experts.{e}.lin_gate.weight"] = r(h, d, scale=d ** -0.5)
        sd[f"routed_experts.{e}.lin2.weight"] = r(d, h, scale=h ** -0.5)
    if ns > 0:
        sd["shared_experts.lin1.weight"] = r(ns, d, h, scale=d ** -0.5)
        sd["shared_experts.lin1.bias"] = r(ns, h, scale=0.2)
        sd["shared_experts.lin2.weight"] = r(ns, h, d, scale=h ** -0.5)
        sd["shared_experts.lin2.bias"] = r(ns, d, scale=0.2)
    sd["gate.weight"] = r(E, d, scale=4 * d ** -0.5)
    sd["gate.bias"] = r(E, scale=0.5)
    sd["biases"] = torch.zeros(E, dtype=dtype) if biases is None else biases.to(dtype)
    return sd
