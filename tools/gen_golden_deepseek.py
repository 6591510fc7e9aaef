"""Generate the DeepSeek-V3 fixtures by running the REFERENCE on the CPU.  Run from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_deepseek.py --ref <path to the reference checkout> [--out tests/golden]

The reference package is imported at run time from ``--ref`` (nothing of it is copied here, and it is never present where the GPU tests
run).  Output, tensors and names only:

  * ``deepseek_tiny.safetensors`` + ``.partK``: inputs, state_dict, main logits, loss and every gradient of
    ``DeepSeekV3Model(TINY_DEEPSEEK).to(bfloat16)`` in bf16 on b = 2, s = 70 (targets include -100), the same of its fp32 twin (same bf16-rounded
    weights, upcast), and for the main block the attention core's inputs and output (q, k as concatenated after RoPE, v, and the context).
  * ``deepseek_mla.safetensors`` + ``.part1``: ``MultiLatentAttention(d_in=32, d_out=128, num_heads=2)`` in bf16 on b = 2, s = 70: state_dict, x, a
    seeded dy, the output, dx and the gradients of ``wk_decoup`` and ``wkv_down_proj``; output, dx and those gradients of the fp32 twin (not its
    weights).  The bf16 weights alone are 0.84 MiB (q_rank = 1536), so with the outputs the fixture is 1.07 MiB and takes two files, each under
    1 MiB.  The only place the reference itself vouches for the shared key's broadcast over two heads.
  * ``deepseek_signatures.json``: constructor parameter names of the classes, state_dict keys with dtypes and shapes, the perturbation seed
    and the floors.

The model test judges a gradient only where the reference's own bf16-vs-twin distance (its floor) is <= 0.1.  ``check_floors`` prints every
floor and fails unless every tensor outside ``deepseek_oracle.FLOOR_ALLOW`` meets it and at most 10 % of the gradient tensors fall outside;
the perturbation seed is the first of ``SEEDS`` for which the reference's numbers alone satisfy that.
"""

import argparse
import contextlib
import inspect
import json
import os
import sys

import torch
from safetensors.torch import save_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 123
SEEDS = range(321, 341)  # candidate seeds of the generator that draws ids, targets and the perturbation
PART_BYTES = 1_000_000  # per file, below the 1 MiB limit for committed files


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@contextlib.contextmanager
def cuda_moves_are_noops():
    """DeepSeekV3Model.forward moves the shifted batches with ``.to("cuda")``; on this CPU run that one call is an identity."""
    orig = torch.Tensor.to

    def to(self, *a, **k):
        if a and a[0] == "cuda":
            return self
        return orig(self, *a, **k)

    torch.Tensor.to = to
    try:
        yield
    finally:
        torch.Tensor.to = orig


class _CatSpy:
    """Stands in for the ``torch`` name inside the reference's attention module while the main block runs: records what ``torch.cat`` returns
    (first the concatenated queries, then the concatenated keys) and forwards everything else."""

    def __init__(self, store):
        self._store = store

    def __getattr__(self, name):
        return getattr(torch, name)

    def cat(self, *a, **k):
        out = torch.cat(*a, **k)
        self._store.setdefault("cats", []).append(out)
        return out


def capture_main_block(m, DA, store):
    blk = m.main_model.trf_blocks[0]
    H = blk.att.num_heads

    def heads(t):
        b, s, d = t.shape
        return t.view(b, s, H, d // H).transpose(1, 2)

    def arm(mod, args):
        DA.torch = _CatSpy(store)

    def disarm(mod, args, out):
        DA.torch = torch

    return [blk.register_forward_pre_hook(arm), blk.register_forward_hook(disarm),
            blk.att.wv_up_proj.register_forward_hook(lambda mod, a, out: store.__setitem__("v", heads(out))),
            blk.att.out_proj.register_forward_pre_hook(lambda mod, a: store.__setitem__("ctx", heads(a[0])))]


def check_floors(t, allowed):
    worst, broken, outside, total = 0.0, [], 0, 0
    floors = {}
    for k in sorted(t):
        if not k.startswith("twin.grad."):
            continue
        name = k[len("twin.grad."):]
        floor = rel_l2(t["grad." + name], t[k])
        floors[name] = floor
        total += 1
        ok = allowed(name)
        print(f"  floor {name}: {floor:.3e}" + ("  (allowed outside)" if ok else ""))
        if floor > 0.1:
            outside += 1
            if not ok:
                broken.append((name, floor))
        if not ok:
            worst = max(worst, floor)
    print(f"  worst floor outside the allow-list: {worst:.3f}; {outside} of {total} gradient tensors above 0.1")
    if outside * 10 > total:
        broken.append(("more than 10 % of the gradient tensors", outside / max(total, 1)))
    return broken, floors


def build_model(DM, DA, cfg, perturb_parameters, input_seed):
    torch.manual_seed(SEED)
    m = DM.DeepSeekV3Model(dict(cfg)).to(torch.bfloat16).train()
    gen = torch.Generator().manual_seed(input_seed)
    b, s, depth = 2, 70, cfg["mtp_depth"]
    tok = torch.randint(0, cfg["vocab_size"], (b, s + 1 + depth), generator=gen)
    ids, tgt = tok[:, :s].contiguous(), tok[:, 1 : s + 1].clone()
    sx = [tok[:, 1 + k : s + 1 + k].contiguous() for k in range(depth)]
    sy = [tok[:, 2 + k : s + 2 + k].clone() for k in range(depth)]
    tgt[1, -5:] = -100  # a padded tail, as the collate function produces
    for k in range(depth):
        sy[k][1, -(6 + k):] = -100
    perturb_parameters(list(m.named_parameters()), gen)
    skip = ("mask", "cos", "sin")  # buffers every implementation derives from the config
    t = {"sd." + k: v for k, v in m.state_dict().items() if k not in skip}
    t["in.ids"], t["in.targets"] = ids, tgt
    for k in range(depth):
        t[f"in.shifted_x.{k}"], t[f"in.shifted_y.{k}"] = sx[k], sy[k]

    cap = {}
    hooks = capture_main_block(m, DA, cap)
    with cuda_moves_are_noops():
        loss = m(ids, tgt, sx, sy)
    for h in hooks:
        h.remove()
    assert DA.torch is torch and len(cap["cats"]) == 2, sorted(cap)
    loss.backward()
    with torch.no_grad():
        logits, _ = m.main_model(ids, m.mask, m.cos, m.sin)
    t["out.logits"], t["out.loss"] = logits, loss
    t.update({"grad." + n: p.grad for n, p in m.named_parameters() if p.grad is not None})
    t.update({"cap.block0.q": cap["cats"][0], "cap.block0.k": cap["cats"][1], "cap.block0.v": cap["v"], "cap.block0.ctx": cap["ctx"]})

    m32 = DM.DeepSeekV3Model(dict(cfg, dtype=torch.float32)).train()
    m32.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in m.state_dict().items()})
    with cuda_moves_are_noops():
        l32 = m32(ids, tgt, sx, sy)
    l32.backward()
    with torch.no_grad():
        logits32, _ = m32.main_model(ids, m32.mask, m32.cos, m32.sin)
    t["twin.logits"], t["twin.loss"] = logits32, l32
    t.update({"twin.grad." + n: p.grad for n, p in m32.named_parameters() if p.grad is not None})
    assert {k[5:] for k in t if k.startswith("grad.")} == {k[10:] for k in t if k.startswith("twin.grad.")}
    return t, m


def build_mla(DA, GlobalBuffers, spec, perturb_parameters):
    torch.manual_seed(SEED)
    att = DA.MultiLatentAttention(d_in=spec["d_in"], d_out=spec["d_out"], num_heads=spec["num_heads"]).to(torch.bfloat16).train()
    gen = torch.Generator().manual_seed(SEEDS[0])
    perturb_parameters(list(att.named_parameters()), gen)
    x = torch.randn(spec["b"], spec["s"], spec["d_in"], generator=gen).to(torch.bfloat16)
    dy = torch.randn(spec["b"], spec["s"], spec["d_out"], generator=gen).to(torch.bfloat16)
    mask = GlobalBuffers.get_causal_mask(spec["context_length"])
    cos, sin = GlobalBuffers.get_rope_params(spec["context_length"], spec["rope_base"], spec["d_out"] // spec["num_heads"] // 2)
    # bf16-rounded tables for both flows, stated here and not left to the state of the reference's table cache (the model twin's load_state_dict
    # writes the rounded buffers into the cached tensors): the bf16 module rounds them anyway, and the twin then computes the same function
    cos, sin = cos.to(torch.bfloat16).float(), sin.to(torch.bfloat16).float()
    t = {"sd." + k: v for k, v in att.state_dict().items()}
    t["in.x"], t["in.dy"] = x, dy
    recorded = ("wk_decoup.weight", "wk_decoup.bias", "wkv_down_proj.weight", "wkv_down_proj.bias")

    def run(mod, xin, dyin, prefix):
        xg = xin.detach().clone().requires_grad_(True)
        y = mod(xg, mask, cos, sin)
        y.backward(dyin)
        t[prefix + "y"], t[prefix + "dx"] = y.detach(), xg.grad
        g = dict(mod.named_parameters())
        t.update({f"{prefix}grad.{n}": g[n].grad for n in recorded})

    run(att, x, dy, "out.")
    att32 = DA.MultiLatentAttention(d_in=spec["d_in"], d_out=spec["d_out"], num_heads=spec["num_heads"]).train()
    att32.load_state_dict({k: v.float() for k, v in att.state_dict().items()})
    run(att32, x.float(), dy.float(), "twin.")
    for n in ("y", "dx") + tuple("grad." + r for r in recorded):
        print(f"  mla floor {n}: {rel_l2(t['out.' + n], t['twin.' + n]):.3e}")
    return t, att


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
    from deepseek_oracle import MLA_FIXTURE, TINY_DEEPSEEK, floor_allowed, perturb_parameters
    from llm_quest.common.buffers import GlobalBuffers
    from llm_quest.llama3_to_deepseekv3 import deepseek_attention as DA
    from llm_quest.llama3_to_deepseekv3 import deepseek_model as DM
    from llm_quest.llama3_to_deepseekv3 import deepseek_transformer_block as DB

    cfg = dict(TINY_DEEPSEEK)
    for seed in SEEDS:
        print(f"perturbation seed {seed}")
        t, m = build_model(DM, DA, cfg, perturb_parameters, seed)
        print(f"loss bf16 {float(t['out.loss'].detach()):.4f}, fp32 twin {float(t['twin.loss'].detach()):.4f}")
        broken, floors = check_floors(t, floor_allowed)
        if not broken:
            break
        print(f"  seed {seed} does not meet the floor condition: {broken}")
    else:
        raise SystemExit("no candidate seed meets the floor condition on the reference's own numbers")
    os.makedirs(args.out, exist_ok=True)
    save_parts(args.out, "deepseek_tiny", t, f"tiny dense DeepSeek-V3 (1 block + 1 MTP module), bf16 + fp32 twin loss and gradients, main-block captures; seed {seed}")

    ta, att = build_mla(DA, GlobalBuffers, MLA_FIXTURE, perturb_parameters)
    save_parts(args.out, "deepseek_mla", ta, "MultiLatentAttention(32, 128, 2) bf16 + fp32 twin outputs and gradients")

    ctor = {}
    for cls in (DA.MultiLatentAttention, DB.RMSNorm, DB.SiLU, DB.FFN, DB.TransformerBlock, DM.MTPModule, DM.MainModel, DM.DeepSeekV3Model):
        ctor[cls.__name__] = [p for p in inspect.signature(cls.__init__).parameters if p != "self"]
    fwd = {cls.__name__: [p for p in inspect.signature(cls.forward).parameters if p != "self"]
           for cls in (DA.MultiLatentAttention, DB.TransformerBlock, DM.MTPModule, DM.MainModel, DM.DeepSeekV3Model)}
    desc = lambda sd: {k: {"dtype": str(v.dtype).replace("torch.", ""), "shape": list(v.shape)} for k, v in sd.items()}
    path = os.path.join(args.out, "deepseek_signatures.json")
    with open(path, "w") as f:
        json.dump({"note": "constructor / forward parameter names and state_dict layouts of the reference's DeepSeek-V3 classes "
                           "(DeepSeekV3Model(TINY_DEEPSEEK).to(bfloat16), MultiLatentAttention(32, 128, 2).to(bfloat16)); generated by tools/gen_golden_deepseek.py",
                   "torch": torch.__version__, "threads": str(torch.get_num_threads()), "constructors": ctor, "forwards": fwd,
                   "state_dict": desc(m.state_dict()), "mla_state_dict": desc(att.state_dict()), "perturbation_seed": seed,
                   "floors": {k: float(f"{v:.4e}") for k, v in floors.items()}}, f, indent=1, sort_keys=True)
    print(f"wrote {path} ({len(m.state_dict())} state_dict keys)")


if __name__ == "__main__":
    main()
