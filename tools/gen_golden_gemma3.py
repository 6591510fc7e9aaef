"""Generate the Gemma3 fixtures by running the REFERENCE on the CPU.  Run from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_gemma3.py --ref <path to the reference checkout> [--out tests/golden]

The reference package is imported at run time from ``--ref`` (nothing of it is copied here, and it is never present where the GPU tests
run).  Output, tensors and names only:

  * ``gemma3_tiny.safetensors`` + ``gemma3_tiny.partK.safetensors``: inputs, state_dict, logits, loss and every gradient of
    ``Gemma3Model(TINY_GEMMA3).to(bfloat16)`` in bf16, the logits, the loss and every gradient of its fp32 twin (same bf16-rounded weights, upcast),
    and for block 1 the input and output of the attention core (q, k, v after RoPE + norm, and the context), of ``post_att_norm`` and the
    FFN's gated product.  Every file stays under 1 MiB; ``tests/gemma3_oracle.py::load_fixture`` reads them back as one dict.
  * ``gemma3_signatures.json``: constructor parameter names of the seven classes, and the state_dict keys with dtypes and shapes.

The model test judges a gradient only where the reference's own bf16-vs-twin distance is <= 0.1 and lets only
``trf_blocks.*.att.k_norm.shift`` fall outside; ``check_floors`` asserts exactly that on the reference's numbers and the generator fails
loudly if it does not hold.
"""

import argparse
import inspect
import json
import os
import sys

import torch
from safetensors.torch import save_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 123
INPUT_SEED = 321  # ids, targets and the perturbation come from a generator of their own
OUTLIER_SUFFIX = ".att.k_norm.shift"
PART_BYTES = 1_000_000  # per file, below the 1 MiB limit for committed files


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def check_floors(t):
    """A constant added to every key moves all scores of a row equally, so the true gradient of k_norm.shift is zero and what the reference
    holds there is rounding noise; every other tensor's floor must be <= 0.1."""
    worst, broken = 0.0, []
    for k in sorted(t):
        if not k.startswith("twin.grad."):
            continue
        name = k[len("twin.grad."):]
        floor = rel_l2(t["grad." + name], t[k])
        outlier = name.endswith(OUTLIER_SUFFIX)
        print(f"  floor {name}: {floor:.3e}" + ("  (allowed outside)" if outlier else ""))
        if not outlier:
            worst = max(worst, floor)
            if floor > 0.1:
                broken.append((name, floor))
    print(f"  worst floor outside k_norm.shift: {worst:.3f}")
    return broken


def capture_block1(m, att_mod, store):
    """Hooks on block 1 (a windowed layer).  q, k, v after RoPE + norm and the context are the arguments and the result of the attention core: the
    module-level windowed function, replaced by a recording wrapper while block 1 runs (k and v arrive repeated to the query heads)."""
    blk = m.trf_blocks[1]
    orig = att_mod.apply_sliding_window_attention

    def spy(queries, keys, values, window_size, swa_mask=None):
        out = orig(queries, keys, values, window_size=window_size, swa_mask=swa_mask)
        store.update(q=queries, k=keys, v=values, ctx=out)
        return out

    def arm(mod, args):
        att_mod.apply_sliding_window_attention = spy

    def disarm(mod, args, out):
        att_mod.apply_sliding_window_attention = orig

    return [blk.register_forward_pre_hook(arm), blk.register_forward_hook(disarm),
            blk.post_att_norm.register_forward_hook(lambda mod, a, out: store.update(post_att_in=a[0], post_att_out=out)),
            blk.ffn.lin2.register_forward_pre_hook(lambda mod, a: store.__setitem__("ffn_prod", a[0]))]


def save_parts(out, stem, tensors, note):
    """The tensors in name order, packed greedily into files of at most PART_BYTES."""
    meta = {"torch": torch.__version__, "threads": str(torch.get_num_threads()), "note": note}
    files, cur, size = [], {}, 0
    for k in sorted(tensors):
        v = tensors[k].detach().clone().contiguous()
        n = v.numel() * v.element_size() + 256
        if cur and size + n > PART_BYTES:
            files.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += n
    files.append(cur)
    for old in os.listdir(out):
        if old.startswith(stem + ".part") and old.endswith(".safetensors"):
            os.remove(os.path.join(out, old))
    for i, f in enumerate(files):
        path = os.path.join(out, stem + (".safetensors" if i == 0 else f".part{i}.safetensors"))
        save_file(f, path, metadata=dict(meta, part=f"{i + 1}/{len(files)}"))
        assert os.path.getsize(path) <= 1 << 20, path
        print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB, {len(f)} tensors)")


def build(G3M, G3A, global_loss, cfg, perturb_parameters):
    torch.manual_seed(SEED)
    m = G3M.Gemma3Model(dict(cfg)).to(torch.bfloat16).train()
    gen = torch.Generator().manual_seed(INPUT_SEED)
    ids = torch.randint(0, cfg["vocab_size"], (2, 70), generator=gen)
    tgt = torch.randint(0, cfg["vocab_size"], (2, 70), generator=gen)
    perturb_parameters(list(m.named_parameters()), gen)
    skip = ("mask", "cos", "sin", "swa_mask", "out_head.weight")  # buffers every implementation derives from the config; the head is the tied embedding
    t = {"sd." + k: v for k, v in m.state_dict().items() if k not in skip}
    t["in.ids"], t["in.targets"] = ids, tgt

    cap = {}
    hooks = capture_block1(m, G3A, cap)
    logits = m(ids)
    for h in hooks:
        h.remove()
    assert sorted(cap) == ["ctx", "ffn_prod", "k", "post_att_in", "post_att_out", "q", "v"], sorted(cap)
    loss = global_loss(logits, tgt, model=m)
    loss.backward()
    t["out.logits"], t["out.loss"] = logits, loss
    t.update({"grad." + n: p.grad for n, p in m.named_parameters()})
    t.update({"cap.block1." + k: v for k, v in cap.items()})

    m32 = G3M.Gemma3Model(dict(cfg, dtype=torch.float32)).train()
    m32.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in m.state_dict().items()})
    logits32 = m32(ids)
    l32 = global_loss(logits32, tgt, model=m32)
    l32.backward()
    t["twin.logits"], t["twin.loss"] = logits32, l32
    t.update({"twin.grad." + n: p.grad for n, p in m32.named_parameters()})
    return t, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project (holds the llm_quest package)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.ref))
    sys.path.insert(1, ROOT)
    sys.path.insert(2, os.path.join(ROOT, "tests"))
    from gemma3_oracle import TINY_GEMMA3, perturb_parameters
    from llm_quest.engine import global_loss
    from llm_quest.llama3_to_gemma3 import gemma3_attention as G3A
    from llm_quest.llama3_to_gemma3 import gemma3_model as G3M
    from llm_quest.llama3_to_gemma3 import gemma3_transformer_block as G3B

    t, m = build(G3M, G3A, global_loss, TINY_GEMMA3, perturb_parameters)
    print(f"loss bf16 {float(t['out.loss'].detach()):.4f}, fp32 twin {float(t['twin.loss'].detach()):.4f}")
    broken = check_floors(t)
    if broken:
        raise SystemExit(f"the reference's own floor exceeds 0.1 outside k_norm.shift: {broken}")
    os.makedirs(args.out, exist_ok=True)
    save_parts(args.out, "gemma3_tiny", t, "tiny Gemma3 (2 windowed layers + 1 global), bf16 + fp32 twin loss and gradients, block-1 captures")

    ctor = {}
    for cls in (G3A.LayerNorm, G3A.GroupedQueryAttention, G3B.RMSNorm, G3B.GELU, G3B.FFN, G3B.TransformerBlock, G3M.Gemma3Model):
        ctor[cls.__name__] = [p for p in inspect.signature(cls.__init__).parameters if p != "self"]
    ctor["apply_sliding_window_attention"] = list(inspect.signature(G3A.apply_sliding_window_attention).parameters)
    sd = {k: {"dtype": str(v.dtype).replace("torch.", ""), "shape": list(v.shape)} for k, v in m.state_dict().items()}
    path = os.path.join(args.out, "gemma3_signatures.json")
    with open(path, "w") as f:
        json.dump({"note": "constructor parameter names and state_dict layout of the reference's Gemma3 classes (Gemma3Model(TINY_GEMMA3).to(bfloat16)); "
                           "generated by tools/gen_golden_gemma3.py", "torch": torch.__version__, "threads": str(torch.get_num_threads()),
                   "constructors": ctor, "state_dict": sd}, f, indent=1, sort_keys=True)
    print(f"wrote {path} ({len(sd)} state_dict keys)")


if __name__ == "__main__":
    main()
