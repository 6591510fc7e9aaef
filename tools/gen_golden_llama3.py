"""Generate the Llama 3.2 / QK-Clip fixtures by running the REFERENCE on the CPU.  Run from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_llama3.py --ref <path to the reference checkout> [--out tests/golden]

The reference package is imported at run time from ``--ref`` (nothing of it is copied here, and it is never present where the GPU tests
run).  Output, tensors and names only:

  * ``llama3_tiny.safetensors`` + ``.partK``: state_dict, inputs (ids, targets, a key mask with sample 1's last 4 keys off), logits with and
    without the mask, loss and every gradient of ``Llama3Model(TINY_LLAMA).to(bfloat16)`` on b = 2, s = 24 (the loss is taken on the masked
    forward); loss, logits and gradients of its fp32 twin (same bf16-rounded weights and buffers, upcast); the per-layer per-head maximum attention
    logits of both forwards, recorded by wrapping ``torch.nn.functional.softmax`` and taking ``amax(dim=(0, 2, 3))`` of its input; ``w_queries`` /
    ``w_keys`` after the reference's ``QKClip(4.0)`` and ``QKClipNaive(4.0)`` on the masked forward's maxima; and, from an MHA twin of the config
    (num_kv_groups = n_heads, same seed), its ``w_queries`` / ``w_keys``, its maxima and the weights after ``MagnitudeQKClipMHA(4.0)``.
  * ``llama3_signatures.json``: constructor and forward parameter names of the model classes, constructor and ``__call__`` parameter names of the
    three clip classes, state_dict keys with dtypes and shapes, the two Llama config dicts without ``dtype``, the seed and the floors.

The model test judges every gradient against the reference's own bf16-vs-twin distance (its floor): the seed is the first of ``SEEDS`` for which every
floor is <= 0.1 on the reference's numbers alone.  No tensor is excluded.
"""

import argparse
import inspect
import json
import os
import sys

import torch
from safetensors.torch import save_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = range(123, 143)
PART_BYTES = 1_000_000  # per file, below the 1 MiB limit for committed files


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


class softmax_inputs:
    """While active, ``torch.nn.functional.softmax`` also records amax(dim=(0, 2, 3)) of its input: the per-head maximum logit of each layer, in
    forward order.  The masked entries (-inf, or finfo.min / 2 with a key mask) never win."""

    def __init__(self):
        self.maxima = []

    def __enter__(self):
        import torch.nn.functional as F

        self._F, self._orig = F, F.softmax

        def spy(x, *a, **k):
            self.maxima.append(torch.amax(x.detach(), dim=(0, 2, 3)).float())
            return self._orig(x, *a, **k)

        F.softmax = spy
        return self

    def __exit__(self, *exc):
        self._F.softmax = self._orig


def qk_weights(m):
    return {f"trf_blocks.{i}.att.{n}.weight": getattr(blk.att, n).weight.detach().clone() for i, blk in enumerate(m.trf_blocks) for n in ("w_queries", "w_keys")}


def clipped(m, clip, maxima):
    """The w_queries / w_keys of every layer after ``clip(m, maxima)``; the model's weights are put back."""
    before = qk_weights(m)
    clip(m, maxima)
    after = qk_weights(m)
    with torch.no_grad():
        for i, blk in enumerate(m.trf_blocks):
            for n in ("w_queries", "w_keys"):
                getattr(blk.att, n).weight.copy_(before[f"trf_blocks.{i}.att.{n}.weight"])
    return after


def build_model(LM, cfg, perturb_parameters, seed):
    torch.manual_seed(seed)
    m = LM.Llama3Model(dict(cfg)).to(torch.bfloat16).train()
    ids = torch.randint(0, cfg["vocab_size"], (2, 24))  # ids, targets and the perturbation from the global generator right after the model, in this order
    tgt = torch.randint(0, cfg["vocab_size"], (2, 24))
    perturb_parameters(list(m.named_parameters()), None)
    km = torch.ones(2, 24, dtype=torch.bool)
    km[1, -4:] = False
    return m, ids, tgt, km


def build(LM, QC, cfg, perturb_parameters, seed, tau):
    m, ids, tgt, km = build_model(LM, cfg, perturb_parameters, seed)
    skip = ("mask", "cos", "sin", "out_head.weight")  # buffers every implementation derives from the config; the head is the tied embedding
    t = {"sd." + k: v for k, v in m.state_dict().items() if k not in skip}
    t["in.ids"], t["in.targets"], t["in.key_mask"] = ids, tgt, km.to(torch.uint8)
    with softmax_inputs() as spy:
        logits = m(ids, km)
    maxima = spy.maxima
    loss = torch.nn.functional.cross_entropy(logits.flatten(0, 1), tgt.flatten())
    loss.backward()
    with torch.no_grad(), softmax_inputs() as spy_nomask:
        t["out.logits_nomask"] = m(ids)
    t["out.logits"], t["out.loss"] = logits, loss
    t.update({"grad." + n: p.grad for n, p in m.named_parameters()})
    for i, (a, b) in enumerate(zip(maxima, spy_nomask.maxima)):
        t[f"out.max_logits.{i}"], t[f"out.max_logits_nomask.{i}"] = a, b
    assert len(maxima) == cfg["n_layers"]

    m32 = LM.Llama3Model(dict(cfg, dtype=torch.float32)).train()
    m32.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in m.state_dict().items()})
    lg32 = m32(ids, km)
    l32 = torch.nn.functional.cross_entropy(lg32.flatten(0, 1), tgt.flatten())
    l32.backward()
    t["twin.logits"], t["twin.loss"] = lg32, l32
    t.update({"twin.grad." + n: p.grad for n, p in m32.named_parameters()})

    for name, after in (("per_head", clipped(m, QC.QKClip(tau), maxima)), ("naive", clipped(m, QC.QKClipNaive(tau), [a.max() for a in maxima]))):
        t.update({f"clip.{name}.{k}": v for k, v in after.items()})

    mha, _, _, _ = build_model(LM, dict(cfg, num_kv_groups=cfg["n_heads"]), perturb_parameters, seed)
    with torch.no_grad(), softmax_inputs() as spy_mha:
        mha(ids, km)
    t.update({"mha.sd." + k: v for k, v in qk_weights(mha).items()})
    for i, a in enumerate(spy_mha.maxima):
        t[f"mha.max_logits.{i}"] = a
    t.update({f"mha.clip.magnitude.{k}": v for k, v in clipped(mha, QC.MagnitudeQKClipMHA(tau), spy_mha.maxima).items()})
    return t, m


def floors_of(t):
    return {k[len("twin.grad."):]: rel_l2(t["grad." + k[len("twin.grad."):]], t[k]) for k in sorted(t) if k.startswith("twin.grad.")}


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
        assert os.path.getsize(path) <= 1 << 20, (path, os.path.getsize(path))
        print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB, {len(f)} tensors)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project (holds the llm_quest package)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.ref))
    sys.path.insert(1, ROOT)
    sys.path.insert(2, os.path.join(ROOT, "tests"))
    import config as ref_config
    from llama3_oracle import FIXTURE_TAU, TINY_LLAMA, perturb_parameters
    from llm_quest.common import qk_clip as QC
    from llm_quest.gpt_to_llama3 import llama_attention as LA
    from llm_quest.gpt_to_llama3 import llama_model as LM
    from llm_quest.gpt_to_llama3 import llama_transformer_block as LB

    cfg = dict(TINY_LLAMA)
    for seed in SEEDS:
        print(f"seed {seed}")
        t, m = build(LM, QC, cfg, perturb_parameters, seed, FIXTURE_TAU)
        floors = floors_of(t)
        print(f"  loss bf16 {float(t['out.loss'].detach()):.4f}, fp32 twin {float(t['twin.loss'].detach()):.4f}; worst floor {max(floors.values()):.4f}")
        for i in range(cfg["n_layers"]):
            print(f"  layer {i} max logits {[round(float(v), 4) for v in t[f'out.max_logits.{i}']]}  mha {[round(float(v), 4) for v in t[f'mha.max_logits.{i}']]}")
        if max(floors.values()) <= 0.1:
            break
        print(f"  seed {seed} does not meet the floor condition")
    else:
        raise SystemExit("no candidate seed meets the floor condition on the reference's own numbers")
    os.makedirs(args.out, exist_ok=True)
    save_parts(args.out, "llama3_tiny", t, f"tiny Llama 3.2 (2 blocks, GQA 4:2, D = 64), bf16 + fp32 twin, max logits, QK-Clip at tau = {FIXTURE_TAU}; seed {seed}")

    params = lambda fn: [p for p in inspect.signature(fn).parameters if p != "self"]
    model_classes = (LA.GroupedQueryAttention, LB.RMSNorm, LB.SiLU, LB.FFN, LB.TransformerBlock, LM.Llama3Model)
    clip_classes = (QC.QKClipNaive, QC.QKClip, QC.MagnitudeQKClipMHA)
    no_dtype = lambda c: {k: v for k, v in c.items() if k != "dtype"}
    desc = lambda sd: {k: {"dtype": str(v.dtype).replace("torch.", ""), "shape": list(v.shape)} for k, v in sd.items()}
    path = os.path.join(args.out, "llama3_signatures.json")
    with open(path, "w") as f:
        json.dump({"note": "constructor / forward parameter names and the state_dict layout of the reference's Llama 3.2 classes (Llama3Model(TINY_LLAMA)"
                           ".to(bfloat16)), constructor / __call__ parameter names of its QK-Clip classes, its two Llama configs; generated by "
                           "tools/gen_golden_llama3.py",
                   "torch": torch.__version__, "threads": str(torch.get_num_threads()),
                   "constructors": {c.__name__: params(c.__init__) for c in model_classes + clip_classes},
                   "forwards": {c.__name__: params(c.forward) for c in model_classes},
                   "calls": {c.__name__: params(c.__call__) for c in clip_classes},
                   "state_dict": desc(m.state_dict()), "seed": seed, "clip_threshold": FIXTURE_TAU,
                   "configs": {"LLAMA32_SMALL_CONFIG_1B": no_dtype(ref_config.LLAMA32_SMALL_CONFIG_1B), "LLAMA32_SMALL_CONFIG": no_dtype(ref_config.LLAMA32_SMALL_CONFIG)},
                   "floors": {k: float(f"{v:.4e}") for k, v in floors.items()}}, f, indent=1, sort_keys=True)
    print(f"wrote {path} ({len(m.state_dict())} state_dict keys)")


if __name__ == "__main__":
    main()
