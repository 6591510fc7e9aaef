"""Plain-torch restatement of the hyper-connection arithmetic (classic "hc"), written from the formulas of the kernels' contract
(include/mi355_vlm.h, csrc/hyper_conn.hip).  TEST INFRASTRUCTURE ONLY: one function per kernel, plus a block and a model.

Every function runs in one of two flows:
  * ``exact=False``: the reference's dtype flow -- bf16 streams, the RMSNorm output rounded to bf16 before it is cast to fp32 for
    the coefficient dot products, fp32 coefficients and mixing, results rounded to bf16 where the reference's ``.to(out_dtype)``
    rounds them.  On the CPU this flow reproduces the reference bit for bit (tests/golden/hyper_qwen3_tiny*.safetensors).
  * ``exact=True``: fp64 throughout, no intermediate rounding -- the value every implementation is measured against.
The backward functions differentiate the forward ones with autograd, as the reference does.

Shapes: X [..., n, d]; ``c`` is a ``Coeffs`` (w_norm [d], W_res [n, d], w_pre / w_post [1, d], f_* [1], b_res [n, n] / b_pre / b_post [n] or None).
"""

import glob
import os
from collections import namedtuple

import torch
import torch.nn.functional as F

Coeffs = namedtuple("Coeffs", "w_norm W_res w_pre w_post f_res f_pre f_post b_res b_pre b_post")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 1e-6


def _cast(c, exact):
    if not exact:
        return c
    return Coeffs(*[None if t is None else t.double() for t in c])


def rmsnorm(x, w, exact=False):
    """x * rsqrt(mean(x^2) + eps) * w in fp32 (fp64), one rstd per (token, stream); rounded to x's dtype in the reference flow."""
    xf = x.double() if exact else x.to(torch.float32)
    inv = torch.rsqrt(xf.pow(2).mean(dim=-1, keepdim=True) + EPS)
    y = xf * inv * (w.double() if exact else w.to(torch.float32))
    return y if exact else y.to(x.dtype)


def coefficients(X, c, exact=False):
    """H [..., n+2, n] (rows: H_res, h_pre, h_post) and the tanh values of the same shape.  H_res[i, j] multiplies stream j into output stream i:
    z_res[i, j] = <xn[j], W_res[i]>."""
    c = _cast(c, exact)
    xn = rmsnorm(X, c.w_norm, exact)
    xn = xn if exact else xn.to(torch.float32)
    th_res = torch.tanh(F.linear(xn, c.W_res).mT)  # [..., j, i] -> [..., i, j]
    th_pre = torch.tanh(F.linear(xn, c.w_pre.reshape(1, -1)).squeeze(-1))
    th_post = torch.tanh(F.linear(xn, c.w_post.reshape(1, -1)).squeeze(-1))
    h_res, h_pre, h_post = th_res * c.f_res, th_pre * c.f_pre, th_post * c.f_post
    if c.b_res is not None:
        h_res = h_res + c.b_res
    if c.b_pre is not None:
        h_pre = h_pre + c.b_pre
    if c.b_post is not None:
        h_post = h_post + c.b_post
    H = torch.cat([h_res, h_pre.unsqueeze(-2), h_post.unsqueeze(-2)], dim=-2)
    TH = torch.cat([th_res, th_pre.unsqueeze(-2), th_post.unsqueeze(-2)], dim=-2)
    return H, TH


def width_fwd(X, c, exact=False):
    """-> R [..., n, d], P [..., d], H, TH."""
    n = X.shape[-2]
    H, TH = coefficients(X, c, exact)
    xf = X.double() if exact else X.to(torch.float32)
    R = H[..., :n, :] @ xf
    P = (H[..., n : n + 1, :] @ xf).squeeze(-2)
    if not exact:
        R, P = R.to(X.dtype), P.to(X.dtype)
    return R, P, H, TH


def depth_fwd(Y, h_post, R, exact=False):
    """Out[..., i, :] = bf16(bf16(h_post[i] * Y) + R[i]) (two roundings in the reference flow)."""
    if exact:
        return h_post.double().unsqueeze(-1) * Y.double().unsqueeze(-2) + R.double()
    return (h_post.unsqueeze(-1) @ Y.unsqueeze(-2).to(torch.float32)).to(Y.dtype) + R


def depth_bwd(dOut, Y, h_post, exact=False):
    """-> dY [..., d], dh_post [..., n] (dR is dOut)."""
    Y = (Y.double() if exact else Y).detach().requires_grad_(True)
    h = (h_post.double() if exact else h_post).detach().requires_grad_(True)
    R = torch.zeros_like(dOut, dtype=torch.float64 if exact else dOut.dtype)
    out = depth_fwd(Y, h, R, exact)
    dY, dh = torch.autograd.grad(out, [Y, h], dOut.double() if exact else dOut)
    return dY, dh


def width_bwd(dR, dP, dh_post, X, c, exact=False):
    """-> dX, dict of parameter gradients (keys: the fields of Coeffs that are not None)."""
    n = X.shape[-2]
    conv = (lambda t: t.double()) if exact else (lambda t: t)
    Xg = conv(X).detach().requires_grad_(True)
    cg = Coeffs(*[None if t is None else conv(t).detach().requires_grad_(True) for t in c])
    R, P, H, _ = width_fwd(Xg, cg, exact)
    names = [k for k in Coeffs._fields if getattr(cg, k) is not None]
    grads = torch.autograd.grad([R, P, H[..., n + 1, :]], [Xg] + [getattr(cg, k) for k in names], [conv(dR), conv(dP), conv(dh_post)])
    return grads[0], dict(zip(names, grads[1:]))


def stream_sum(X, exact=False):
    return X.double().sum(dim=-2) if exact else X.sum(dim=-2)


def stream_broadcast(x, n):
    return x.unsqueeze(-2).expand(*x.shape[:-1], n, x.shape[-1])


# --------------------------------------------------------------------------------------------------------------- block and model (reference flow)
def coeffs_from_sd(sd, pfx):
    """Coeffs of one sub-block from a state_dict (``pfx`` = 'trf_blocks.1.hc_attn.')."""
    g = lambda k: sd.get(pfx + k)
    return Coeffs(g("norm.weight"), g("res.linear.weight"), g("pre.linear.weight"), g("post.linear.weight"), g("res.factor"), g("pre.factor"),
                  g("post.factor"), g("res.bias"), g("pre.bias"), g("post.bias"))


def block(sd, pfx, x, cfg, cos, sin, capture=None):
    """HyperQwen3TransformerBlock on x [b, s, n, d]; ``capture`` (a dict) receives X, R, P, Y, Out of both halves under 'attn.' / 'ffn.'."""
    from oracle import models, ops

    for half in ("attn", "ffn"):
        c = coeffs_from_sd(sd, f"{pfx}hc_{half}.")
        n = x.shape[-2]
        R, P, H, _ = width_fwd(x, c)
        if half == "attn":
            Y = models.qwen3_attention(sd, pfx + "att.", ops.rmsnorm(P, sd[pfx + "norm1.weight"]), cfg, cos, sin)
        else:
            Y = ops.swiglu_ffn(ops.rmsnorm(P, sd[pfx + "norm2.weight"]), sd[pfx + "ffn.lin1.weight"], sd[pfx + "ffn.lin_gate.weight"],
                               sd[pfx + "ffn.lin2.weight"])
        out = depth_fwd(Y, H[..., n + 1, :], R)
        if capture is not None:
            capture.update({f"{half}.X": x, f"{half}.R": R, f"{half}.P": P, f"{half}.Y": Y, f"{half}.Out": out})
        x = out
    return x


def model(sd, cfg, ids, n, capture_block=None, capture=None):
    """HyperQwen3Model.forward: logits [b, s, vocab]."""
    from oracle import ops

    cos, sin = ops.rope_tables(cfg["rope_base"], cfg["head_dim"], cfg["context_length"])
    x = stream_broadcast(F.embedding(ids, sd["emb_dict.weight"]), n)
    for i in range(cfg["n_layers"]):
        x = block(sd, f"trf_blocks.{i}.", x, cfg, cos, sin, capture if i == capture_block else None)
    x = ops.rmsnorm(stream_sum(x), sd["final_norm.weight"])
    head = sd["out_head.weight"] if "out_head.weight" in sd else sd["emb_dict.weight"]
    return F.linear(x, head)


# --------------------------------------------------------------------------------------------------------------- fixture and operands
def load_fixture():
    """tests/golden/hyper_qwen3_tiny.safetensors and its .partK continuation files (every committed file stays under 1 MiB) as one dict."""
    from safetensors.torch import load_file

    t = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, "hyper_qwen3_tiny*.safetensors"))):
        t.update(load_file(path))
    if not t:
        raise FileNotFoundError("tests/golden/hyper_qwen3_tiny*.safetensors")
    return t


def perturb_coefficients(named_parameters, gen=None):
    """Move every coefficient off its initial value (at initialisation H_res = I and every dynamic weight is 0, which tests nothing):
    linear.weight ~ N(0, 0.05), factor = 0.3, bias += 0.1 * N(0, 1), drawn in parameter order from ``gen`` (default: torch's global generator).
    Used by the fixture generator."""
    with torch.no_grad():
        for k, p in named_parameters:
            if ".hc_attn." not in "." + k and ".hc_ffn." not in "." + k:
                continue
            if k.endswith("linear.weight"):
                p.copy_(torch.randn(p.shape, generator=gen) * 0.05)
            elif k.endswith(".factor"):
                p.fill_(0.3)
            elif k.endswith(".bias"):
                p.add_(0.1 * torch.randn(p.shape, generator=gen))


def make_operands(T, n, d, seed, bias=True):
    """Seeded kernel operands: X ~ N(0, 1) with one stream scaled by 8 and one by 1/8, coefficients as in the fixture recipe."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(T, n, d, generator=g)
    X[:, 0] *= 8.0
    X[:, n - 1] *= 0.125
    rn = lambda *s: torch.randn(*s, generator=g)
    c = Coeffs(
        w_norm=(1.0 + 0.1 * rn(d)).to(torch.bfloat16), W_res=0.05 * rn(n, d), w_pre=0.05 * rn(1, d), w_post=0.05 * rn(1, d),
        f_res=torch.tensor([0.3]), f_pre=torch.tensor([0.3]), f_post=torch.tensor([0.3]),
        b_res=torch.eye(n) + 0.1 * rn(n, n) if bias else None, b_pre=torch.ones(n) / n + 0.1 * rn(n) if bias else None,
        b_post=torch.ones(n) + 0.1 * rn(n) if bias else None,
    )
    Y = rn(T, d).to(torch.bfloat16)
    dOut = rn(T, n, d).to(torch.bfloat16)
    dP = rn(T, d).to(torch.bfloat16)
    dh_post = rn(T, n)
    return X.to(torch.bfloat16), c, Y, dOut, dP, dh_post


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))
