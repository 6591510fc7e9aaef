"""Generate the Reinforced Attention Learning fixtures by running the REFERENCE on the CPU in fp32.  Run from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_ral.py --ref <path to the reference checkout> [--out tests/golden]

The reference module is imported at run time from ``--ref`` (nothing of it is copied here, and it is never present where the GPU tests run).
Output, tensors and names only:

  * ``ral_reference.safetensors``: per case ``<case>.policy`` / ``.old`` (attention weights [b, h, s, s]), ``.adv`` [b], ``.loss_mask`` [b, s],
    ``.ral_factor`` [1], ``.loss_fn`` (``attention_divergence_loss``), ``.loss_cls`` (``AttentionDivergenceLoss``), ``.grad_fn`` / ``.grad_cls`` (the
    gradient of each with respect to the policy weights) and ``.P`` (``_prepare_attention_weights`` of the policy weights).  Cases: ``inline``, the
    reference's own inline example (seed 42, b, h, s = 2, 2, 3), and a few with s <= 65: causal softmaxes with padded keys, and one dense.
  * ``ral_signatures.json``: the parameter names and defaults of the constructor, the methods and the function.

Also prints the reference's own fp32-vs-fp64 gap per case (what the tolerance of tests/test_ral_cpu.py sits two orders above).
"""

import argparse
import inspect
import json
import os
import sys

import torch
from safetensors.torch import save_file

CASES = (  # name, b, h, s, kind, ral_factor
    ("causal33", 2, 4, 33, "causal_right", 1.0),
    ("causal65", 2, 3, 65, "causal_left", 0.7),
    ("dense48", 1, 2, 48, "dense", 1.3),
)


def weights(b, h, s, kind, g):
    sc = 2.0 * torch.randn(b, h, s, s, generator=g)
    if kind != "dense":
        hidden = torch.ones(s, s, dtype=torch.bool).triu_(1).expand(b, 1, s, s).clone()
        if kind == "causal_right":
            hidden[0, :, :, s - s // 3:] = True
        else:
            hidden[0, :, :, : s // 3] = True
        sc = sc.masked_fill(hidden, torch.finfo(torch.float32).min / 2)  # a fully hidden row attends uniformly, as the reference's models leave it
    return torch.softmax(sc, dim=-1)


def run(R, policy, old, adv, loss_mask, factor, dtype):
    out = {}
    c = lambda t: t.to(dtype) if t.is_floating_point() else t
    for form in ("fn", "cls"):
        p = c(policy).detach().requires_grad_(True)
        if form == "fn":
            loss = R.attention_divergence_loss(p, c(old), c(adv), loss_mask, ral_factor=factor)
        else:
            m = R.AttentionDivergenceLoss(ral_factor=factor)
            m.precompute_q_and_mask(c(old))
            loss = m(p, c(adv), loss_mask)
        (grad,) = torch.autograd.grad(loss, p)
        out["loss_" + form], out["grad_" + form] = loss.detach().reshape(1), grad
    eye = torch.eye(policy.shape[-1], dtype=torch.bool)
    out["P"] = R.AttentionDivergenceLoss._prepare_attention_weights(c(policy), eye)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
    a = ap.parse_args()
    sys.path.insert(0, a.ref)
    from llm_quest.common import reinforced_attention_learning as R

    t = {}
    inputs = {}
    # the reference's inline example, draw for draw
    torch.manual_seed(42)
    b, h, s = 2, 2, 3
    policy = torch.softmax(torch.randn(b, h, s, s), dim=-1)
    old = torch.softmax(torch.randn(b, h, s, s), dim=-1)
    adv = torch.randn(2)
    inputs["inline"] = (policy, old, adv, torch.tensor([[1, 1, 0], [1, 0, 0]]), 1.0)
    g = torch.Generator().manual_seed(20260204)
    for name, b, h, s, kind, factor in CASES:
        lm = torch.ones(b, s, dtype=torch.int64)
        lm[:, : s // 4] = 0
        inputs[name] = (weights(b, h, s, kind, g), weights(b, h, s, kind, g), torch.randn(b, generator=g), lm, factor)
    rel = lambda x, y: float((x.double() - y).norm() / y.norm().clamp_min(1e-300))
    for name, (policy, old, adv, lm, factor) in inputs.items():
        r32, r64 = (run(R, policy, old, adv, lm, factor, dt) for dt in (torch.float32, torch.float64))
        t.update({f"{name}.policy": policy, f"{name}.old": old, f"{name}.adv": adv, f"{name}.loss_mask": lm, f"{name}.ral_factor": torch.tensor([factor])})
        t.update({f"{name}.{k}": v for k, v in r32.items()})
        print(f"{name}: fp32 vs fp64  loss {rel(r32['loss_fn'], r64['loss_fn']):.2e}  grad {rel(r32['grad_fn'], r64['grad_fn']):.2e}  "
              f"class vs function (fp32) loss {rel(r32['loss_cls'], r32['loss_fn'].double()):.2e} grad {rel(r32['grad_cls'], r32['grad_fn'].double()):.2e}")
    path = os.path.join(a.out, "ral_reference.safetensors")
    save_file({k: v.contiguous() for k, v in t.items()}, path)
    print(path, os.path.getsize(path), "bytes")

    def params(fn):
        return [[n, None if p.default is inspect.Parameter.empty else p.default] for n, p in inspect.signature(fn).parameters.items() if n != "self"]

    C = R.AttentionDivergenceLoss
    sig = {"AttentionDivergenceLoss": {"__init__": params(C.__init__), "precompute_q_and_mask": params(C.precompute_q_and_mask),
                                       "_prepare_attention_weights": params(C._prepare_attention_weights), "forward": params(C.forward)},
           "attention_divergence_loss": params(R.attention_divergence_loss),
           "static_methods": ["_prepare_attention_weights"],
           "forward_before_precompute": "We must call `precompute_qlog_q` before calling `forward`."}
    with open(os.path.join(a.out, "ral_signatures.json"), "w") as f:
        json.dump(sig, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
