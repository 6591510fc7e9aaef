"""Plain-torch restatement of the Nemotron-3 LatentMoE arithmetic: the sigmoid router with balancing biases and a scaling factor, the squared-ReLU
GLU, an expert and the layer, written from the formulas of the kernels' contract (include/mi355_vlm.h, csrc/latent_moe.hip).  TEST INFRASTRUCTURE ONLY.

Every function runs in one of two flows, chosen by ``dtype`` (as tests/deepseek_moe_oracle.py, whose helpers are imported, not copied):
  * ``dtype=None``: the reference's dtype flow on the tensors as given -- for bf16 tensors every torch op rounds its result to bf16 where the
    reference's modules do (the gate's matmul, the sigmoid, the biased key in the promoted dtype of p and the buffer, the sum of the selected
    probabilities, the division by it and the in-place scaling; every expert's two products, relu, square and the gated product; every routed
    expert's output times its weight and the latent accumulator after EVERY expert's ``index_add_``, experts ascending; the up projection and the
    add onto the shared expert's output); for fp32 tensors the same ops in fp32;
  * ``dtype=torch.float64``: everything upcast first, no intermediate rounding -- the value every implementation is measured against.
The top-k selection is explicit: the k largest keys in descending order, the lower expert index first among equal keys.  The selection is a constant
of the backward; ``biases`` carries no gradient.  Where a selection enters, ``idx`` gives one to evaluate on.
"""

import torch
import torch.nn.functional as F

from deepseek_moe_oracle import GOLDEN, _c, bias_update, biased_key, boundary_tie, counts_of, load_fixture, rel_l2, topk_lowest_index_first  # noqa: F401

BF16 = torch.bfloat16

# the two fixture layers (tools/gen_golden_latent_moe.py): emb_dim 64 (latent 16), hidden sizes that are no multiple of 32, input (2, 35, 64)
FIXTURE_CFG = dict(emb_dim=64, moe_hidden_dim=40, shared_expert_hidden_dim=48, dtype=BF16)
FIXTURE_LAYERS = {
    "A": dict(kwargs=dict(top_k=1, num_experts=3), E=12, k=4, to_bf16=False),  # padded gate, fp32 biases from plain construction
    "B": dict(kwargs=dict(), E=16, k=8, to_bf16=True),  # the upstream defaults after .to(bfloat16): bf16 biases
}
FIXTURE_BATCH, FIXTURE_SEQ = 2, 35
SCALING, RATE = 2.5, 1e-3


def bias_pattern(E):
    """Layer A's balancing biases: fp32 values that bf16 cannot hold, large against the gaps between neighbouring probabilities."""
    return torch.tensor([0.0625 * ((3 * e % 5) - 2) + 1e-4 * (e + 1) for e in range(E)], dtype=torch.float32)


# ----------------------------------------------------------------------------------------------------------------- router
def route(logits, biases, k, scaling, dtype=None, idx=None):
    """-> (p [T, E], idx int64 [T, k], w [T, k], s [T]) (nvidia_latent_moe.py:101-108).  ``idx``: a selection to use instead of this flow's own."""
    x = _c(logits, dtype)
    p = torch.sigmoid(x)
    if idx is None:
        _, idx = topk_lowest_index_first(biased_key(p, _c(biases, dtype)), k)
    v = p.gather(1, idx)
    s = v.sum(dim=-1, keepdim=True)
    w = v / s
    w = w * scaling
    return p, idx, w, s.squeeze(-1)


def route_bwd(logits, biases, k, scaling, dw, dtype=None, idx=None):
    x = _c(logits, dtype).detach().requires_grad_(True)
    _, _, w, _ = route(x, biases, k, scaling, dtype=dtype, idx=idx)
    return torch.autograd.grad((w * _c(dw, w.dtype)).sum(), x)[0]


def key_boundary_tie(logits, biases, k):
    """Rows whose k-th and (k+1)-th largest BIASED keys are equal (reference dtype flow)."""
    return boundary_tie(biased_key(torch.sigmoid(logits), biases), k)


def logits_without_boundary_tie(T, E, k, biases, seed, std=1.0):
    """bf16 logits [T, E] ~ N(0, std), every row redrawn until its biased keys have no tie at the k-th / (k+1)-th place.  ``std`` keeps the sigmoid
    off saturation: near 1 the bf16 probabilities are 2^-8 apart and most rows of a wide layer would tie."""
    g = torch.Generator().manual_seed(seed)
    x = (std * torch.randn(T, E, generator=g)).to(BF16)
    for _ in range(256):
        bad = key_boundary_tie(x, biases, k)
        if not bool(bad.any()):
            return x
        x[bad] = (std * torch.randn(int(bad.sum()), E, generator=g)).to(BF16)
    raise RuntimeError("could not draw tie-free logits")


def _ulp_move(x, up):
    bits = x.view(torch.int16).to(torch.int32)
    step = torch.where((x >= 0) == up, 1, -1)
    moved = (bits + step).to(torch.int16).view(BF16)
    tiny = torch.tensor(2.0 ** -133, dtype=torch.float32).to(BF16)
    return torch.where(x == 0, tiny if up else -tiny, moved)


def robust_tokens(logits, biases, k):
    """[T] bool: the selected SET survives a move of every bf16 logit by one bf16 ulp in the worst direction -- the selected experts' logits one ulp
    down and all others one ulp up (a sigmoid does not couple experts) -- judged on the keys of the reference dtype flow."""
    E = logits.shape[1]
    _, idx0 = topk_lowest_index_first(biased_key(torch.sigmoid(logits), biases), k)
    sel = torch.zeros_like(logits, dtype=torch.bool).scatter_(1, idx0, True)
    if k >= E:
        return torch.ones(logits.shape[0], dtype=torch.bool)
    worst = torch.where(sel, _ulp_move(logits, False), _ulp_move(logits, True))
    key = biased_key(torch.sigmoid(worst), biases).float()
    lo_sel = key.masked_fill(~sel, float("inf")).min(dim=1).values
    hi_rest = key.masked_fill(sel, float("-inf")).max(dim=1).values
    return lo_sel > hi_rest


# ----------------------------------------------------------------------------------------------------------------- activation, expert
def relu2_glu(gu, dtype=None):
    """a = u * relu(g)^2 on the fused pair [u | g] (nvidia_latent_moe.py:14, 44)."""
    x = _c(gu, dtype)
    F_ = x.shape[1] // 2
    return x[:, :F_] * torch.square(torch.relu(x[:, F_:]))


def relu2_glu_grads(gu, da, dtype=None):
    """-> (a, dgu [R, 2F] = [du | dg])."""
    x = _c(gu, dtype).detach().requires_grad_(True)
    a = relu2_glu(x)
    return a.detach(), torch.autograd.grad(a, x, _c(da, dtype))[0]


def expert(x, w1, wg, w2):
    """Expert.forward (nvidia_latent_moe.py:39-44): lin2(lin1(x) * relu(lin_gate(x))^2)."""
    return F.linear(F.linear(x, w1) * torch.square(torch.relu(F.linear(x, wg))), w2)


def expert_grads(x, w1, wg, w2, dy, dtype=None):
    """-> (y, dx, d lin1, d lin_gate, d lin2)."""
    ops = [_c(t, dtype).detach().requires_grad_(True) for t in (x, w1, wg, w2)]
    y = expert(*ops)
    return (y.detach(),) + tuple(torch.autograd.grad(y, ops, _c(dy, dtype)))


# ----------------------------------------------------------------------------------------------------------------- the layer
def layer(sd, x2d, k, scaling=SCALING, rate=RATE, dtype=None, idx=None, record=None):
    """LatentMoE.forward on [T, d] with the buffer ``sd['biases']`` as it stands BEFORE the forward -> (out [T, d], idx [T, k]).  The dispatch is
    upstream's, statement for statement (the rows of an expert in ``torch.where(expert_mask[e])`` order).  ``record`` (a dict) receives logits, p,
    idx, w, counts and the biases a training forward leaves."""
    E = sd["gate.weight"].shape[0]
    x = _c(x2d, dtype)
    g = lambda name: _c(sd[name], dtype)
    ex = lambda pre, v: expert(v, g(pre + "lin1.weight"), g(pre + "lin_gate.weight"), g(pre + "lin2.weight"))
    out = ex("shared_expert.", x)
    x_lat = F.linear(x, g("down_proj.weight"))
    routed = torch.zeros_like(x_lat)
    logits = F.linear(x, g("gate.weight"))
    biases = sd["biases"].detach()
    p, idx, w, _ = route(logits, biases, k, scaling, idx=idx)
    mask = F.one_hot(idx, num_classes=E).permute(2, 1, 0)
    for e in range(E):
        pos, tok = torch.where(mask[e])
        if tok.numel() == 0:
            continue
        routed = routed.index_add(0, tok, ex(f"routed_experts.{e}.", x_lat[tok]) * w[tok, pos].unsqueeze(-1))
    out = out + F.linear(routed, g("up_proj.weight"))
    if record is not None:
        counts = counts_of(idx, E)
        record.update(out=out.detach(), logits=logits.detach(), p=p.detach(), idx=idx, w=w.detach(), counts=counts, biases=bias_update(biases, counts, rate))
    return out, idx


def layer_grads(sd, x2d, k, dy, scaling=SCALING, dtype=None, idx=None):
    """-> (out, dx, {name: gradient}, idx) under the upstream gradient ``dy``; an expert without a token has a zero gradient."""
    leaves = {n: _c(v, dtype).detach().requires_grad_(True) for n, v in sd.items() if n != "biases"}
    xg = _c(x2d, dtype).detach().requires_grad_(True)
    out, idx = layer({**sd, **leaves}, xg, k, scaling, idx=idx)
    names = list(leaves)
    grads = torch.autograd.grad(out, [xg] + [leaves[n] for n in names], _c(dy, dtype), allow_unused=True)
    return out.detach(), grads[0], {n: (torch.zeros_like(leaves[n]) if g is None else g) for n, g in zip(names, grads[1:])}, idx


def loss_grad(out):
    """d/d(out) of the fixture's loss ``out.float().square().mean()``, in ``out``'s dtype (what autograd hands the layer)."""
    return (2.0 * out.float() / out.numel()).to(out.dtype)
