"""Generate the classic-MoE fixture by running the REFERENCE on the CPU.  Run from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_classic_moe.py --ref <path to the reference checkout> [--out tests/golden]

The reference package is imported at run time from ``--ref`` (nothing of it is copied here, and it is never present where the GPU tests run).
Output, tensors and names only:

  * ``classic_moe_tiny.safetensors`` (+ ``.partK``, each under 1 MiB): two layers on input (2, 35, emb_dim), keys prefixed ``A.`` / ``B.``:
      A  ``MoE(dict(emb_dim=80), num_experts=3, top_k=1, scaling_factor=0.125)``: hidden 40 (no multiple of 32), a gate that needs padding;
      B  ``MoE(dict(emb_dim=64))``: the upstream defaults, 8 experts, top-2, "auto", hidden 128.
    Both after ``.to(bfloat16)``, with weights and biases perturbed off their initial values (``perturb``).  Per layer: ``in.x``, the state_dict
    (``sd.*``), ``topk_idxs``, the output ``out``, ``moe_loss``, the upstream gradient ``in.dout`` and the loss weight ``in.g`` of the total
    ``(out * dout).sum() + g * moe_loss``, every gradient (``grad.x``, ``grad.<parameter>``; an expert without a token has none), and the same from
    the fp32 twin (same bf16-rounded weights, upcast) with the bf16 run's selection forced (``twin.*``).
  * ``classic_moe_signatures.json``: constructor parameter names and defaults, state_dict keys with dtypes and shapes, the chosen seeds, the floors.

Conditions (not measurements) that the reference's own numbers must meet; per layer the seed is the first of 0, 1, 2, ... that meets them, and it is
stored:
  * no token has a boundary tie between its k-th and (k+1)-th probability;
  * the distance of the reference's bf16 run to its fp32 twin is at most 0.1 for the output, the loss and every gradient.
"""

import argparse
import importlib.util
import inspect
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = range(0, 64)
GATE_SCALE = 4.0  # as initialised the probabilities crowd around 1 / E, where every token sits on a near-tie
G_LOSS = 8.0  # the loss weight, and
DOUT_SCALE = 2.0 ** -6  # the upstream gradient's scale: with top_k = 1 the weights are the constant 1, so the output's share of the gate's gradient is pure
# bf16 rounding noise (1 / s and v / s^2 round apart); the loss's share has to stand well above it for the gate's floors to mean anything


def _moe_generator():
    spec = importlib.util.spec_from_file_location("gen_golden_deepseek_moe", os.path.join(ROOT, "tools", "gen_golden_deepseek_moe.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def perturb(m, gen):
    """Off the initial values: the gate sharpened, every bias moved by 0.1 N(0, 1) (the gate's by 0.5), every expert weight by 10 % of its own scale."""
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n == "gate.weight":
                p.mul_(GATE_SCALE)
            elif n == "gate.bias":
                p.add_((0.5 * torch.randn(p.shape, generator=gen)).to(p.dtype))
            elif n.endswith("bias"):
                p.add_((0.1 * torch.randn(p.shape, generator=gen)).to(p.dtype))
            else:
                p.add_((0.1 * float(p.float().std()) * torch.randn(p.shape, generator=gen)).to(p.dtype))


def build(CM, CO, GM, spec, seed):
    cfg, k = dict(spec["cfg"]), spec["k"]
    torch.manual_seed(seed)
    m = CM.MoE(cfg, **spec["kwargs"]).to(torch.bfloat16).train()
    assert (m.num_experts, m.top_k, m.experts[0].hidden_dim) == (spec["E"], k, spec["hidden"])
    assert (m.load_coeff, m.z_router_coeff) == (CO.LOAD_COEFF, CO.Z_COEFF)
    gen = torch.Generator().manual_seed(seed)
    perturb(m, gen)
    shape = (CO.FIXTURE_BATCH, CO.FIXTURE_SEQ, cfg["emb_dim"])
    x = torch.randn(shape, generator=gen).to(torch.bfloat16)
    dout = (DOUT_SCALE * torch.randn(shape, generator=gen)).to(torch.bfloat16)
    sd0 = {n: v.detach().clone() for n, v in m.state_dict().items()}
    t = {"sd." + n: v for n, v in sd0.items()}
    t["in.x"], t["in.dout"], t["in.g"] = x, dout, torch.tensor(G_LOSS)

    rec = {}
    h = m.gate.register_forward_hook(lambda mod, a, out: rec.update(logits=out.detach().clone()))
    xg = x.clone().requires_grad_(True)
    out = m(xg)
    h.remove()
    ((out * dout).sum() + G_LOSS * m.moe_loss).backward()
    assert m.moe_loss.dim() == 0 and m.moe_loss.dtype == torch.bfloat16
    t["out"], t["moe_loss"], t["grad.x"], t["logits"] = out.detach(), m.moe_loss.detach().clone(), xg.grad, rec["logits"]
    t.update({"grad." + n: p.grad for n, p in m.named_parameters() if p.grad is not None})
    p = torch.nn.functional.softmax(rec["logits"], dim=-1)
    idx = p.topk(k, dim=-1)[1]  # the reference's own expression on the reference's own tensors: the selection it made
    t["topk_idxs"] = idx.to(torch.int32)
    ties = int(CO.boundary_tie(p, k).sum())

    m32 = CM.MoE(cfg, **spec["kwargs"]).train()
    m32.load_state_dict({n: v.float() for n, v in sd0.items()})
    x32 = x.float().requires_grad_(True)
    queue = [idx]
    with GM.forced_topk(queue):
        out32 = m32(x32)
    assert not queue
    ((out32 * dout.float()).sum() + G_LOSS * m32.moe_loss).backward()
    t["twin.out"], t["twin.moe_loss"], t["twin.grad.x"] = out32.detach(), m32.moe_loss.detach().clone(), x32.grad
    t.update({"twin.grad." + n: q.grad for n, q in m32.named_parameters() if q.grad is not None})
    assert {n[5:] for n in t if n.startswith("grad.")} == {n[10:] for n in t if n.startswith("twin.grad.")}
    floors = {n[10:]: CO.rel_l2(t["grad." + n[10:]], v) for n, v in t.items() if n.startswith("twin.grad.")}
    floors["out"] = CO.rel_l2(t["out"], t["twin.out"])
    floors["moe_loss"] = CO.rel_l2(t["moe_loss"], t["twin.moe_loss"])
    worst = max(floors, key=floors.get)
    counts = torch.bincount(idx.view(-1), minlength=spec["E"])
    print(f"  {ties} boundary ties, counts {counts.tolist()}, largest floor {floors[worst]:.3e} ({worst})")
    broken = []
    if ties:
        broken.append(("boundary ties", ties))
    if floors[worst] > 0.1:
        broken.append((f"floor of {worst}", floors[worst]))
    return t, sd0, broken, floors


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project (holds the llm_quest package)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.ref))
    sys.path.insert(1, ROOT)
    sys.path.insert(2, os.path.join(ROOT, "tests"))
    import classic_moe_oracle as CO
    from llm_quest.moe import classic_moe as CM

    GM = _moe_generator()
    tensors, layout, seeds, floors = {}, {}, {}, {}
    desc = lambda sd: {k: {"dtype": str(v.dtype).replace("torch.", ""), "shape": list(v.shape)} for k, v in sd.items()}
    for name, spec in CO.FIXTURE_LAYERS.items():
        for seed in SEEDS:
            print(f"layer {name}, seed {seed}")
            t, sd0, broken, fl = build(CM, CO, GM, spec, seed)
            if not broken:
                break
            print(f"  seed {seed} does not meet the conditions: {broken}")
        else:
            raise SystemExit(f"layer {name}: no candidate seed meets the conditions on the reference's own numbers")
        assert not broken and not bool(CO.boundary_tie(torch.nn.functional.softmax(t["logits"], dim=-1), spec["k"]).any()) and max(fl.values()) <= 0.1
        tensors.update({f"{name}.{k}": v for k, v in t.items()})
        layout[name], seeds[name], floors[name] = desc(sd0), seed, {k: float(f"{v:.4e}") for k, v in fl.items()}
    os.makedirs(args.out, exist_ok=True)
    GM._dense_generator().save_parts(args.out, "classic_moe_tiny", tensors,
                                     f"two classic MoE layers (A: emb 80, 3 experts, top-1, hidden 40; B: emb 64, 8 experts, top-2, hidden 128), bf16 + fp32 twin (forced selection); seeds {seeds}")
    required = "<required>"
    ctor = {cls.__name__: {n: (required if q.default is inspect.Parameter.empty else q.default) for n, q in inspect.signature(cls.__init__).parameters.items() if n != "self"}
            for cls in (CM.ExpertGeLU, CM.MoE, CM.MoE_old)}
    path = os.path.join(args.out, "classic_moe_signatures.json")
    with open(path, "w") as f:
        json.dump({"note": "constructor parameters (in order, with defaults) and state_dict layout of the reference's classic MoE classes (layers A and B of "
                           "classic_moe_oracle.FIXTURE_LAYERS); generated by tools/gen_golden_classic_moe.py",
                   "torch": torch.__version__, "threads": str(torch.get_num_threads()), "constructors": ctor, "constructor_order": {c: list(v) for c, v in ctor.items()},
                   "state_dict": layout, "seed": seeds, "gate_scale": GATE_SCALE, "g_loss": G_LOSS, "dout_scale": DOUT_SCALE, "floors": floors}, f, indent=1, sort_keys=True)
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
