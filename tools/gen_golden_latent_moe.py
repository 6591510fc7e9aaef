"""Generate the LatentMoE fixture by running the REFERENCE on the CPU.  Run from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_latent_moe.py --ref <path to the reference checkout> [--out tests/golden]

The reference package is imported at run time from ``--ref`` (nothing of it is copied here, and it is never present where the GPU tests run).
Output, tensors and names only:

  * ``latent_moe_tiny.safetensors`` (+ ``.partK``, each under 1 MiB): two layers on emb_dim 64 (latent 16), moe_hidden_dim 40, shared hidden 48, input
    (2, 35, 64), keys prefixed ``A.`` / ``B.``:
      A  ``LatentMoE(cfg, top_k=1, num_experts=3)``: 12 experts, top_k 4, a gate that needs padding, fp32 ``biases`` from plain construction set to
         a pattern bf16 cannot hold (``latent_moe_oracle.bias_pattern``);
      B  the upstream defaults (16 experts, top_k 8) after ``.to(bfloat16)``: bf16 ``biases``, a bf16-exact pattern.
    Per layer: ``in.x``, the state_dict before the forward (``sd.*``), the gate's ``logits``, ``topk_idxs``, ``counts``, the updated ``biases``, the
    output ``out``, every gradient under the loss ``out.float().square().mean()`` (``grad.x``, ``grad.<parameter>``; an expert without a token has none),
    the same from the fp32 twin (same bf16-rounded weights, upcast) with the bf16 run's selection forced (``twin.*``), and the per-token flag ``robust``.
  * ``latent_moe_signatures.json``: constructor parameter names, state_dict keys with dtypes and shapes, the chosen seeds, the floors.

Conditions (not measurements) that the reference's own numbers must meet; per layer the seed is the first of ``SEEDS`` that meets them:
  * no token has a boundary tie in the biased key;
  * the non-zero ``biases`` change at least one selection;
  * at least 90 % of the tokens are robust (``latent_moe_oracle.robust_tokens``).
The gate's weights are scaled by ``GATE_SCALE``: as initialised the probabilities crowd around 0.5, times 8 the sigmoid saturates to exactly 1.0.
"""

import argparse
import importlib.util
import inspect
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = range(521, 561)
GATE_SCALE = 2.0


def _moe_generator():
    spec = importlib.util.spec_from_file_location("gen_golden_deepseek_moe", os.path.join(ROOT, "tools", "gen_golden_deepseek_moe.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build(LM, LO, GM, spec, seed):
    cfg = dict(LO.FIXTURE_CFG)
    E, k = spec["E"], spec["k"]
    torch.manual_seed(seed)
    m = LM.LatentMoE(cfg, **spec["kwargs"])
    if spec["to_bf16"]:
        m = m.to(torch.bfloat16)
    m.train()
    assert (m.num_experts, m.top_k) == (E, k) and m.biases.dtype == (torch.bfloat16 if spec["to_bf16"] else torch.float32)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(LO.FIXTURE_BATCH, LO.FIXTURE_SEQ, cfg["emb_dim"], generator=gen).to(torch.bfloat16)
    with torch.no_grad():
        m.gate.weight.mul_(GATE_SCALE)
        pattern = LO.bias_pattern(E)
        m.biases.copy_((pattern - 1e-4 * torch.arange(1, E + 1)).to(torch.bfloat16) if spec["to_bf16"] else pattern)
    sd0 = {n: v.detach().clone() for n, v in m.state_dict().items()}
    b0 = sd0["biases"]
    assert bool((b0 != 0).any()) and (spec["to_bf16"] or bool((b0.to(torch.bfloat16).float() != b0).any()))
    t = {"sd." + n: v for n, v in sd0.items()}
    t["in.x"] = x

    rec = {}
    h = m.gate.register_forward_hook(lambda mod, a, out: rec.update(logits=out.detach().clone()))
    xg = x.clone().requires_grad_(True)
    out = m(xg)
    h.remove()
    out.float().square().mean().backward()
    t["out"], t["grad.x"], t["biases"], t["logits"] = out.detach(), xg.grad, m.biases.detach().clone(), rec["logits"]
    t.update({"grad." + n: p.grad for n, p in m.named_parameters() if p.grad is not None})

    p = torch.sigmoid(rec["logits"])
    idx = (p + b0).topk(k, dim=-1)[1]  # the reference's own expression on the reference's own tensors: the selection it made
    idx_plain = p.topk(k, dim=-1)[1]
    counts = torch.bincount(idx.view(-1), minlength=E)
    assert torch.equal(LO.bias_update(b0, counts, m.bias_update_rate), t["biases"]), "the recomputed selection does not reproduce the reference's bias update"
    ties = int(LO.key_boundary_tie(rec["logits"], b0, k).sum())
    moved = int((idx.sort(dim=1).values != idx_plain.sort(dim=1).values).any(dim=1).sum())
    robust = LO.robust_tokens(rec["logits"], b0, k)
    saturated = int((p == 1).sum())
    print(f"  {ties} boundary ties, biases change {moved} selections, {int(robust.sum())} of {robust.numel()} tokens robust, {saturated} probabilities at 1.0, counts {counts.tolist()}")
    broken = []
    if ties:
        broken.append(("boundary ties", ties))
    if not moved:
        broken.append(("the biases change no selection", 0))
    if int(robust.sum()) * 10 < 9 * robust.numel():
        broken.append(("robust tokens", float(robust.float().mean())))
    t["topk_idxs"], t["counts"], t["robust"] = idx.to(torch.int32), counts.to(torch.int32), robust.to(torch.uint8)

    m32 = LM.LatentMoE(dict(cfg, dtype=torch.float32), **spec["kwargs"]).train()
    m32.load_state_dict({n: v.float() for n, v in sd0.items()})
    x32 = x.float().requires_grad_(True)
    queue = [idx]
    with GM.forced_topk(queue):
        out32 = m32(x32)
    assert not queue
    out32.float().square().mean().backward()
    t["twin.out"], t["twin.grad.x"] = out32.detach(), x32.grad
    t.update({"twin.grad." + n: p.grad for n, p in m32.named_parameters() if p.grad is not None})
    assert {n[5:] for n in t if n.startswith("grad.")} == {n[10:] for n in t if n.startswith("twin.grad.")}
    floors = {n[10:]: LO.rel_l2(t["grad." + n[10:]], v) for n, v in t.items() if n.startswith("twin.grad.")}
    floors["out"] = LO.rel_l2(t["out"], t["twin.out"])
    return t, sd0, broken, floors


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project (holds the llm_quest package)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.ref))
    sys.path.insert(1, ROOT)
    sys.path.insert(2, os.path.join(ROOT, "tests"))
    import latent_moe_oracle as LO
    from llm_quest.moe import nvidia_latent_moe as LM

    GM = _moe_generator()
    tensors, layout, seeds, floors = {}, {}, {}, {}
    desc = lambda sd: {k: {"dtype": str(v.dtype).replace("torch.", ""), "shape": list(v.shape)} for k, v in sd.items()}
    for name, spec in LO.FIXTURE_LAYERS.items():
        for seed in SEEDS:
            print(f"layer {name}, seed {seed}")
            t, sd0, broken, fl = build(LM, LO, GM, spec, seed)
            if not broken:
                break
            print(f"  seed {seed} does not meet the conditions: {broken}")
        else:
            raise SystemExit(f"layer {name}: no candidate seed meets the conditions on the reference's own numbers")
        tensors.update({f"{name}.{k}": v for k, v in t.items()})
        layout[name], seeds[name], floors[name] = desc(sd0), seed, {k: float(f"{v:.4e}") for k, v in fl.items()}
    os.makedirs(args.out, exist_ok=True)
    GM._dense_generator().save_parts(args.out, "latent_moe_tiny", tensors,
                                     f"two LatentMoE layers (A: 12 experts, top_k 4, fp32 biases; B: 16 experts, top_k 8, bf16 biases), bf16 + fp32 twin (forced selection); seeds {seeds}")
    ctor = {cls.__name__: [p for p in inspect.signature(cls.__init__).parameters if p != "self"] for cls in (LM.SquaredReLU, LM.Expert, LM.LatentMoE)}
    path = os.path.join(args.out, "latent_moe_signatures.json")
    with open(path, "w") as f:
        json.dump({"note": "constructor parameter names and state_dict layout of the reference's LatentMoE classes (layers A and B of "
                           "latent_moe_oracle.FIXTURE_LAYERS); generated by tools/gen_golden_latent_moe.py",
                   "torch": torch.__version__, "threads": str(torch.get_num_threads()), "constructors": ctor, "state_dict": layout, "seed": seeds,
                   "gate_scale": GATE_SCALE, "floors": floors}, f, indent=1, sort_keys=True)
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
