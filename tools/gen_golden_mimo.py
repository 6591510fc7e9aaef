"""Generate the MiMo-V2-Flash fixture by running the REFERENCE on the CPU.  Run from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_mimo.py --ref <path to the reference checkout> [--out tests/golden]

The reference package is imported at run time from ``--ref`` (nothing of it is copied here, and it is never present where the GPU tests run).
Output, tensors and names only:

  * ``mimo_tiny.safetensors`` + ``.partK`` (each under 1 MiB, at most 12 files): inputs, state_dict (``biases`` as they stand BEFORE the forward: a
    non-zero pattern), main logits, loss and every gradient of ``MiMoModel(TINY_MIMO).to(bfloat16)`` (GA-dense, SWA-MoE, GA-MoE, SWA-MoE and two MTP
    modules) on b = 2, s = 70 with -100 among the targets; per MoE layer ``moe.<layer>.``: the layer input ``x`` and output ``out``, the gate's
    ``logits``, ``topk_idxs``, ``counts``, the updated ``biases``, ``max_vio`` and the per-token flag ``robust``; for layer 1 (SWA) and layer 2 (GA)
    ``cap.<layer>.``: q and k after norm + RoPE, v and the context; and logits, loss and gradients of the fp32 twin (same bf16-rounded weights and
    tables, upcast), run with the bf16 run's ``topk_idxs`` forced.
  * ``mimo_signatures.json``: constructor parameter names and defaults, forward parameter names, state_dict keys with dtypes and shapes, the chosen
    seed, the floors.

Conditions (not measurements) that the reference's own numbers must meet; the seed is the first of ``SEEDS`` that meets them:
  * no token of any MoE layer has a boundary tie in the biased key;
  * the non-zero ``biases`` change at least one selection per MoE layer;
  * at least 90 % of the tokens of the first MoE layer are robust (``deepseek_moe_oracle.robust_tokens``);
  * every parameter receives a gradient (no routed expert is left without a token);
  * every gradient's bf16-vs-twin distance is at most 0.1 outside ``mimo_oracle.FLOOR_ALLOW``, with at most 10 % of the tensors above it.
"""

import argparse
import importlib.util
import inspect
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 123
SEEDS = range(721, 761)
MAX_FILES = 12
CAPTURED = (1, 2)  # one sliding-window and one global-attention layer


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def bias_pattern(E, layer):
    """Non-zero balancing biases as ``gen_golden_deepseek_moe.bias_pattern`` draws them -- large against the gaps between neighbouring probabilities,
    different per layer, bf16-exact -- but with a value of its own per expert (odd multiples of 1/64 for E = 8): with top_k = 2 of 8 and a sharpened
    gate most probabilities round to nothing against their bias, and two experts sharing one bias would then tie on every such token."""
    return torch.tensor([(2 * ((e * 3 + layer) % E) - (E - 1)) / 64.0 for e in range(E)])


class _RopeSpy:
    """Stands in for the ``RoPE`` name inside the reference's attention module while a captured layer runs: records what ``RoPE.apply`` returns
    (first the queries, then the keys) and forwards everything else."""

    def __init__(self, real, store):
        self._real, self._store = real, store

    def __getattr__(self, name):
        return getattr(self._real, name)

    def apply(self, *a, **k):
        out = self._real.apply(*a, **k)
        self._store.setdefault("roped", []).append(out.detach().clone())
        return out


def capture_attention(MA, att, store):
    real = MA.RoPE

    def heads(t, width):
        b, s, d = t.shape
        return t.view(b, s, d // width, width).transpose(1, 2).detach().clone()

    def arm(mod, args):
        MA.RoPE = _RopeSpy(real, store)

    def disarm(mod, args, out):
        MA.RoPE = real

    return [att.register_forward_pre_hook(arm), att.register_forward_hook(disarm),
            att.w_values.register_forward_hook(lambda mod, a, out: store.__setitem__("v", heads(out, att.value_head_dim))),
            att.out_proj.register_forward_pre_hook(lambda mod, a: store.__setitem__("ctx", heads(a[0], att.value_head_dim)))]


def build(MM, MA, MOE, GM, MO, O, cfg, seed):
    torch.manual_seed(SEED)
    m = MM.MiMoModel(dict(cfg)).to(torch.bfloat16).train()
    gen = torch.Generator().manual_seed(seed)
    b, s = O.FIXTURE_BATCH, O.FIXTURE_SEQ
    tok = torch.randint(0, cfg["vocab_size"], (b, s + 1), generator=gen)
    ids, tgt = tok[:, :s].contiguous(), tok[:, 1:].clone()
    tgt[1, -5:] = -100  # a padded tail, as the collate function produces
    O.perturb_parameters(list(m.named_parameters()), gen)
    layers = O.moe_layers(cfg)
    with torch.no_grad():
        for i in layers:
            ffn = m.main_model.layers[i].feed_forward
            assert isinstance(ffn, MOE.DeepSeekMoE)
            ffn.gate.weight.mul_(8.0)  # fresh gate weights give near-uniform probabilities, where every token sits on a near-tie
            ffn.biases.copy_(bias_pattern(ffn.num_routed, i).to(ffn.biases.dtype))
    skip = ("main_model.mask_swa", "main_model.mask_ga", "main_model.cos_swa", "main_model.sin_swa", "main_model.cos_ga", "main_model.sin_ga")
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    t = {"sd." + k: v for k, v in sd0.items() if k not in skip}  # the buffers every implementation derives from the config stay out
    t["in.ids"], t["in.targets"] = ids, tgt

    rec, cap, hooks, main_logits = {i: {} for i in layers}, {i: {} for i in CAPTURED}, [], []
    for i in layers:
        ffn = m.main_model.layers[i].feed_forward
        hooks.append(ffn.register_forward_pre_hook(lambda mod, a, i=i: rec[i].update(x=a[0].detach().clone(), b0=mod.biases.detach().clone())))
        hooks.append(ffn.gate.register_forward_hook(lambda mod, a, out, i=i: rec[i].update(logits=out.detach().clone())))
        hooks.append(ffn.register_forward_hook(lambda mod, a, out, i=i: rec[i].update(out=out.detach().clone(), biases=mod.biases.detach().clone(),
                                                                                      max_vio=mod.max_vio.detach().clone())))
    for i in CAPTURED:
        hooks += capture_attention(MA, m.main_model.layers[i].att, cap[i])
    hooks.append(m.main_model.out_head.register_forward_hook(lambda mod, a, out: main_logits.append(out.detach().clone())))
    loss = m(ids, tgt)
    for h in hooks:
        h.remove()
    loss.backward()
    t["out.logits"], t["out.loss"] = main_logits[0], loss
    missing = [n for n, p in m.named_parameters() if p.grad is None]  # an expert that received no token
    t.update({"grad." + n: p.grad for n, p in m.named_parameters() if p.grad is not None})
    for i in CAPTURED:
        assert len(cap[i]["roped"]) == 2, (i, sorted(cap[i]))
        t[f"cap.{i}.q"], t[f"cap.{i}.k"], t[f"cap.{i}.v"], t[f"cap.{i}.ctx"] = cap[i]["roped"][0], cap[i]["roped"][1], cap[i]["v"], cap[i]["ctx"]

    broken, queue = [], []
    if missing:
        broken.append(("parameters without a gradient", missing[:3]))
    for i in layers:
        r, k = rec[i], cfg["top_k"]
        logits = r["logits"].reshape(-1, r["logits"].shape[-1])
        E = logits.shape[1]
        p = torch.nn.functional.softmax(logits, dim=-1)
        idx = (p + r["b0"]).topk(k, dim=-1)[1]  # the reference's own expression on the reference's own tensors: the selection it made
        idx_plain = p.topk(k, dim=-1)[1]
        counts = torch.bincount(idx.view(-1), minlength=E)
        want = r["b0"].clone()
        want += cfg["moe_bias_update_rate"] * (counts.float().mean() - counts.float()).sign()
        assert torch.equal(want, r["biases"]), "the recomputed selection does not reproduce the reference's bias update"
        ties = int(MO.key_boundary_tie(logits, r["b0"], k).sum())
        moved = int((idx.sort(dim=1).values != idx_plain.sort(dim=1).values).any(dim=1).sum())
        robust = MO.robust_tokens(logits, r["b0"], k)
        print(f"  layer {i}: {ties} boundary ties, biases change {moved} selections, {int(robust.sum())} of {robust.numel()} tokens robust, counts {counts.tolist()}")
        if ties:
            broken.append((f"layer {i}: boundary ties", ties))
        if not moved:
            broken.append((f"layer {i}: the biases change no selection", 0))
        if i == layers[0] and int(robust.sum()) * 10 < 9 * robust.numel():
            broken.append((f"layer {i}: robust tokens", float(robust.float().mean())))
        pre = f"moe.{i}."
        t[pre + "x"], t[pre + "out"], t[pre + "logits"] = r["x"].reshape(-1, r["x"].shape[-1]), r["out"].reshape(-1, r["out"].shape[-1]), logits
        t[pre + "topk_idxs"], t[pre + "counts"] = idx.to(torch.int32), counts.to(torch.int32)
        t[pre + "biases"], t[pre + "max_vio"], t[pre + "robust"] = r["biases"], r["max_vio"].float().reshape(1), robust.to(torch.uint8)
        queue.append(idx)

    m32 = MM.MiMoModel(dict(cfg, dtype=torch.float32)).train()
    m32.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in sd0.items()})
    twin_logits = []
    h = m32.main_model.out_head.register_forward_hook(lambda mod, a, out: twin_logits.append(out.detach().clone()))
    with GM.forced_topk(queue):
        l32 = m32(ids, tgt)
    h.remove()
    assert not queue
    l32.backward()
    t["twin.logits"], t["twin.loss"] = twin_logits[0], l32
    t.update({"twin.grad." + n: p.grad for n, p in m32.named_parameters() if p.grad is not None})
    assert {k[5:] for k in t if k.startswith("grad.")} == {k[10:] for k in t if k.startswith("twin.grad.")}
    return t, m, sd0, broken


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project (holds the llm_quest package)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.ref))
    sys.path.insert(1, ROOT)
    sys.path.insert(2, os.path.join(ROOT, "tests"))
    import deepseek_moe_oracle as MO
    import mimo_oracle as O
    from llm_quest.moe import deepseek_moe as MOE
    from llm_quest.xiaomi import mimo_v2_flash_attention as MA
    from llm_quest.xiaomi import mimo_v2_flash_model as MM
    from llm_quest.xiaomi import mimo_v2_flash_transformer_block as MB

    G, GM = _tool("gen_golden_deepseek"), _tool("gen_golden_deepseek_moe")
    cfg = dict(O.TINY_MIMO)
    for seed in SEEDS:
        print(f"seed {seed}")
        t, m, sd0, broken = build(MM, MA, MOE, GM, MO, O, cfg, seed)
        print(f"loss bf16 {float(t['out.loss'].detach()):.4f}, fp32 twin {float(t['twin.loss'].detach()):.4f}")
        more, floors = G.check_floors(t, O.floor_allowed)
        broken += more
        if not broken:
            break
        print(f"  seed {seed} does not meet the conditions: {broken}")
    else:
        raise SystemExit("no candidate seed meets the conditions on the reference's own numbers")
    os.makedirs(args.out, exist_ok=True)
    G.save_parts(args.out, "mimo_tiny", t, f"tiny MiMo-V2-Flash (GA-dense, SWA-MoE, GA-MoE, SWA-MoE, 2 MTP modules), bf16 + fp32 twin (forced selection); seed {seed}")
    files = [f for f in os.listdir(args.out) if f.startswith("mimo_tiny") and f.endswith(".safetensors")]
    assert len(files) <= MAX_FILES, f"{len(files)} fixture files, at most {MAX_FILES} allowed"

    classes = (MA.GroupedQueryAttentionWithSink, MB.FFN, MB.TransformerBlock, MM.MTPModule, MM.MainModel, MM.MiMoModel)
    jsonable = lambda v: v if isinstance(v, (type(None), bool, int, float, str)) else repr(v)
    ctor, defaults = {}, {}
    for cls in classes:
        params = [p for n, p in inspect.signature(cls.__init__).parameters.items() if n != "self"]
        ctor[cls.__name__] = [p.name for p in params]
        defaults[cls.__name__] = {p.name: jsonable(p.default) for p in params if p.default is not inspect.Parameter.empty}
    fwd = {cls.__name__: [p for p in inspect.signature(cls.forward).parameters if p != "self"] for cls in classes}
    desc = lambda sd: {k: {"dtype": str(v.dtype).replace("torch.", ""), "shape": list(v.shape)} for k, v in sd.items()}
    path = os.path.join(args.out, "mimo_signatures.json")
    with open(path, "w") as f:
        json.dump({"note": "constructor / forward parameter names and state_dict layout of the reference's MiMo-V2-Flash classes "
                           "(MiMoModel(TINY_MIMO).to(bfloat16)); generated by tools/gen_golden_mimo.py",
                   "torch": torch.__version__, "threads": str(torch.get_num_threads()), "constructors": ctor, "constructor_defaults": defaults,
                   "forwards": fwd, "state_dict": desc(sd0), "seed": seed, "floors": {k: float(f"{v:.4e}") for k, v in floors.items()}},
                  f, indent=1, sort_keys=True)
    print(f"wrote {path} ({len(sd0)} state_dict keys)")


if __name__ == "__main__":
    main()
