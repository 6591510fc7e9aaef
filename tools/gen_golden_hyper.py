"""Generate the hyper-connection fixtures by running the REFERENCE on the CPU.  Run from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_hyper.py --ref <path to the reference checkout> [--out tests/golden]

The reference package is imported at run time from ``--ref`` (nothing of it is copied here, and it is never present where the GPU tests
run).  Output, tensors and names only:

  * ``hyper_qwen3_tiny.safetensors`` + ``hyper_qwen3_tiny.partK.safetensors``: inputs, state_dict, logits, loss and every gradient of
    ``HyperQwen3Model(TINY_QWEN, "hc", 4)`` in bf16, the loss and every gradient of its fp32 twin (same weights upcast), and X, R, P, Y,
    Out of both sub-blocks of block 1 (the second block, where the streams differ).  The tensors are spread over several files so that
    no committed file exceeds 1 MiB; ``tests/hyper_oracle.py::load_fixture`` reads them back as one dict.
  * ``hyper_signatures.json``: constructor parameter names of the five classes, and the state_dict keys with dtypes and shapes.

Metadata as ``oracle/gen_golden.py`` writes it (torch version, thread count, note).
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
N_STREAMS = 4
PART_BYTES = 1_000_000  # per file, below the 1 MiB limit for committed files
MAX_PERTURB_SEEDS = 32
OUTLIERS_ALLOWED = ("trf_blocks.0.hc_attn.pre.",)  # see check_floors


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def capture_block(blk, store):
    """Hooks on one HyperQwen3TransformerBlock: X / R (res in, out), P (pre out), Y (post in) per sub-block; Out of the attention half is what
    the FFN half's norm receives, Out of the FFN half is the block's output."""
    hooks = []
    for half, hc in (("attn", blk.hc_attn), ("ffn", blk.hc_ffn)):
        def res_hook(mod, args, out, half=half):
            store[f"{half}.X"], store[f"{half}.R"] = args[0], out
        def pre_hook(mod, args, out, half=half):
            store[f"{half}.P"] = out
        def post_hook(mod, args, out, half=half):
            store[f"{half}.Y"] = args[0]
        hooks += [hc["res"].register_forward_hook(res_hook), hc["pre"].register_forward_hook(pre_hook), hc["post"].register_forward_hook(post_hook)]
    hooks.append(blk.hc_ffn["norm"].register_forward_pre_hook(lambda mod, args: store.__setitem__("attn.Out", args[0])))
    hooks.append(blk.register_forward_hook(lambda mod, args, out: store.__setitem__("ffn.Out", out)))
    return hooks


def check_floors(t):
    """The 1.5x rule judges a gradient only where the reference's own bf16-vs-fp32 distance is <= 0.1.  Above that sit only the three
    trf_blocks.0.hc_attn.pre.* tensors: in block 0 every stream is a copy of the embedding, so P is a scalar multiple of it and norm1 right
    behind it is scale-invariant -- the true gradient is ~0 and what remains is rounding noise.  Returns the names that break this.

    Whether it holds depends on the draw: the gradient of a scalar ``factor`` is a sum over all tokens with heavy cancellation, and with the
    perturbation drawn from torch's global generator right after the model (seed 123) the reference's own floor is 0.22 for
    trf_blocks.1.hc_attn.post.factor and 0.12 for trf_blocks.1.hc_attn.pre.factor.  A fixture on which the reference itself is that noisy is no
    yardstick, so the perturbation has a generator of its own and main() takes the FIRST seed 0, 1, 2, ... whose fixture meets the condition.  The
    choice looks at the reference's numbers only; the seed is stored as in.perturb_seed."""
    above = []
    for k in sorted(t):
        if k.startswith("twin.grad."):
            name = k[len("twin.grad."):]
            floor = rel_l2(t["grad." + name], t[k])
            if floor > 0.1:
                above.append((name, floor))
    for name, floor in above:
        print(f"  floor above 0.1: {name} {floor:.3f}")
    return [n for n, _ in above if not n.startswith(OUTLIERS_ALLOWED)]


def save_parts(out, stem, tensors, note):
    meta = {"torch": torch.__version__, "threads": str(torch.get_num_threads()), "note": note}
    flat = {k: v.detach().clone().contiguous() for k, v in tensors.items()}
    nbytes = lambda v: v.numel() * v.element_size() + 256
    small = {k: v for k, v in flat.items() if nbytes(v) < 40_000}
    big = sorted(((k, v) for k, v in flat.items() if k not in small), key=lambda kv: kv[0])
    files, cur, size = [small], {}, 0
    assert sum(nbytes(v) for v in small.values()) < PART_BYTES
    for k, v in big:
        if size + nbytes(v) > PART_BYTES and cur:
            files.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += nbytes(v)
    if cur:
        files.append(cur)
    for old in os.listdir(out):
        if old.startswith(stem + ".part") and old.endswith(".safetensors"):
            os.remove(os.path.join(out, old))
    for i, f in enumerate(files):
        path = os.path.join(out, stem + (".safetensors" if i == 0 else f".part{i}.safetensors"))
        save_file(f, path, metadata=dict(meta, part=f"{i + 1}/{len(files)}"))
        assert os.path.getsize(path) <= 1 << 20, path
        print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB, {len(f)} tensors)")


def build(HQ, global_loss, TINY_QWEN, perturb_coefficients, pseed):
    torch.manual_seed(SEED)
    m = HQ.HyperQwen3Model(dict(TINY_QWEN), hc_type="hc", expansion_rate=N_STREAMS).to(torch.bfloat16).train()
    ids = torch.randint(0, TINY_QWEN["vocab_size"], (2, 24))
    tgt = torch.randint(0, TINY_QWEN["vocab_size"], (2, 24))
    perturb_coefficients(list(m.named_parameters()), torch.Generator().manual_seed(pseed))
    skip = ("mask", "cos", "sin", "out_head.weight")  # buffers every implementation derives from the config; the head is the tied embedding
    t = {"sd." + k: v for k, v in m.state_dict().items() if k not in skip}
    t["in.ids"], t["in.targets"] = ids, tgt
    t["in.perturb_seed"] = torch.tensor([pseed])
    cap = {}
    hooks = capture_block(m.trf_blocks[1], cap)
    logits = m(ids)
    for h in hooks:
        h.remove()
    loss = global_loss(logits, tgt, model=m)
    loss.backward()
    t["out.logits"], t["out.loss"] = logits, loss
    t.update({"grad." + n: p.grad for n, p in m.named_parameters()})
    t.update({"cap.block1." + k: v for k, v in cap.items()})
    assert len(cap) == 10, sorted(cap)

    cfg32 = dict(TINY_QWEN, dtype=torch.float32)
    m32 = HQ.HyperQwen3Model(cfg32, hc_type="hc", expansion_rate=N_STREAMS).train()
    m32.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in m.state_dict().items()})
    l32 = global_loss(m32(ids), tgt, model=m32)
    l32.backward()
    t["twin.loss"] = l32
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
    from hyper_oracle import perturb_coefficients
    from llm_quest.common.hyper_connections import hyper_connections as HC
    from llm_quest.common.hyper_connections import hyper_qwen3 as HQ
    from llm_quest.engine import global_loss
    from oracle.gen_golden import TINY_QWEN

    for pseed in range(MAX_PERTURB_SEEDS):
        print(f"perturbation seed {pseed}:")
        t, m = build(HQ, global_loss, TINY_QWEN, perturb_coefficients, pseed)
        if not check_floors(t):
            break
    else:
        raise SystemExit(f"no perturbation seed below {MAX_PERTURB_SEEDS} meets the floor condition")
    os.makedirs(args.out, exist_ok=True)
    save_parts(args.out, "hyper_qwen3_tiny", t, "tiny HyperQwen3 (hc, n = 4), bf16 + fp32 twin loss and gradients, block-1 captures")

    ctor = {}
    for cls in (HC.HyperConnectionRes, HC.HyperConnectionPre, HC.HyperConnectionPost, HQ.HyperQwen3TransformerBlock, HQ.HyperQwen3Model):
        ctor[cls.__name__] = [p for p in inspect.signature(cls.__init__).parameters if p != "self"]
    sd = {k: {"dtype": str(v.dtype).replace("torch.", ""), "shape": list(v.shape)} for k, v in m.state_dict().items()}
    path = os.path.join(args.out, "hyper_signatures.json")
    with open(path, "w") as f:
        json.dump({"note": "constructor parameter names and state_dict layout of the reference's hyper-connection classes (HyperQwen3Model(TINY_QWEN, 'hc', 4)"
                           ".to(bfloat16)); generated by tools/gen_golden_hyper.py", "torch": torch.__version__, "threads": str(torch.get_num_threads()),
                   "constructors": ctor, "state_dict": sd}, f, indent=1, sort_keys=True)
    print(f"wrote {path} ({len(sd)} state_dict keys)")


if __name__ == "__main__":
    main()
