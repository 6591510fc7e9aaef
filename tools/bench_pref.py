"""Measure preference tuning on the GPU: a DPO step through the logits against one from the hidden states, and the reward pooling kernels against torch ops.

    python tools/bench_pref.py [--pairs 8] [--seq 512] [--size 0.6B] [--steps 5] [--warmup 2] [--rounds 3] [--pool 64 512 1024]
                               [--out profiles/pref_bench.json]

DPO: Qwen3-0.6B as policy and as reference model, ``pairs`` preference pairs of ``seq`` positions (a ``dpo_collate`` batch of synthetic token lists).  The two
variants alternate inside one process, ``--rounds`` times each, forward + ``backward()``:

  a. ``forward``: one concatenated (2 pairs, seq) pass per model to the (2 pairs, seq, vocab) logits;
  b. ``forward_from_hidden``: one concatenated (2 pairs, seq) pass per model, the LM head walked in vocabulary chunks (the default ``vocab_chunk``).

Pooling: the four modes of ``PrefRewardCalculator`` on bf16 hidden states ``--pool`` = (b, s, emb) with an fp32 head, forward + backward, each against the same
expression in torch ops (what the reference runs).  ``scores_mean`` takes the head's (b, s, 1) output as its operand, so the head's N = 1 GEMM is outside its timing
and inside ``scores_from_hidden``'s.

Times are device events around whole calls, medians after warm-up, no profiler attached; a variant's figure is the median of its rounds' medians and every round's
median is kept.  ``peak_bytes`` is the rise of ``torch.cuda.max_memory_allocated`` over one call above the level in front of it (weights, attached gradients and
workspaces already allocated).  Reported, not gated.  One JSON line per measurement on stdout, all of them in ``--out``.  Needs the GPU.
"""

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))
sys.path.insert(2, os.path.join(ROOT, "tests"))

from bench_deepseek_moe import time_calls  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32


def _rounds(variants, steps, warmup, rounds, dev):
    runs = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            runs[name].append(time_calls(fn, steps, warmup))
    out = {}
    for name, fn in variants:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        fn()
        torch.cuda.synchronize()
        meds = sorted(r["ms_median"] for r in runs[name])
        out[name] = dict(ms_median=meds[len(meds) // 2], ms_min=min(r["ms_min"] for r in runs[name]), ms_max=max(r["ms_max"] for r in runs[name]),
                         round_ms_medians=[r["ms_median"] for r in runs[name]], peak_bytes=torch.cuda.max_memory_allocated(dev) - base)
    return out


def measure_dpo(pairs, seq, size, steps, warmup, rounds):
    from llm_quest_amd.alignment.dpo.dpo import DPOLoss
    from llm_quest_amd.config import qwen3_config_creator
    from llm_quest_amd.dataset import dpo_collate
    from llm_quest_amd.qwen.qwen3.qwen3_model import Qwen3Model

    dev = torch.device("cuda", 0)
    cfg = dict(qwen3_config_creator(size), context_length=seq)
    torch.manual_seed(0)
    with torch.device(dev):
        policy, reference = Qwen3Model(cfg).train(), Qwen3Model(cfg).eval()
    gen = torch.Generator().manual_seed(1)
    V = cfg["vocab_size"]
    items = []
    for i in range(pairs):
        prompt = torch.randint(1, V, (seq // 8 + i,), generator=gen).tolist()
        items.append({"prompt": prompt, "chosen": prompt + torch.randint(1, V, (seq - 1 - len(prompt) - 3 * i,), generator=gen).tolist(),
                      "rejected": prompt + torch.randint(1, V, (seq - 1 - len(prompt) - 5 * ((i + 1) % pairs),), generator=gen).tolist()})
    batch = dpo_collate(items, pad_token_id=0, device=dev)
    assert tuple(batch["chosen"].shape) == (pairs, seq)
    loss_fn = DPOLoss()

    def run(fn):
        def step():
            policy.zero_grad(set_to_none=False)
            fn(batch, policy, reference)[0].backward()

        return step

    res = _rounds([("forward", run(loss_fn.forward)), ("forward_from_hidden", run(loss_fn.forward_from_hidden))], steps, warmup, rounds, dev)
    out = [dict(bench="pref_dpo", variant=name, model=f"Qwen3-{size}", pairs=pairs, seq=seq, vocab=V, steps=steps, rounds=rounds, **r) for name, r in res.items()]
    out.append(dict(bench="pref_dpo", variant="ratios", logits_bytes_2b_s_v=2 * pairs * seq * V * 2,
                    from_hidden_over_forward_ms=res["forward_from_hidden"]["ms_median"] / res["forward"]["ms_median"],
                    from_hidden_over_forward_peak=res["forward_from_hidden"]["peak_bytes"] / max(res["forward"]["peak_bytes"], 1)))
    return out


def measure_pool(B, S, E, steps, warmup, rounds):
    import pref_oracle as PO
    from llm_quest_amd.alignment.rlhf_grpo.grpo_engine import PrefRewardCalculator as P

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    hid = torch.randn(B, S, E, generator=g, device=dev).to(BF16).requires_grad_(True)
    head = torch.nn.Linear(E, 1).to(dev)
    lens = torch.randint(S // 2, S + 1, (B,), generator=g, device=dev)
    attn = torch.arange(S, device=dev).expand(B, S) < lens.unsqueeze(1)
    mask = attn & (torch.arange(S, device=dev).expand(B, S) >= S // 8)
    scores = torch.randn(B, S, 1, generator=g, device=dev).requires_grad_(True)
    w, b = head.weight, head.bias

    def step(fn):
        def run():
            hid.grad = scores.grad = w.grad = b.grad = None
            fn().sum().backward()

        return run

    hf = lambda: hid.float()  # the torch expressions run the head in fp32 on the bf16 hidden states, as the kernels accumulate
    pairs = {"scores_mean": (lambda: P.scores_mean_pooling(scores, mask), lambda: PO.scores_mean(scores, mask)),
             "hidden_mean": (lambda: P.hidden_states_mean_pooling(hid, mask, head), lambda: PO.hidden_mean(hf(), mask, w, b)),
             "last_token": (lambda: P.last_token_score(hid, attn, head), lambda: PO.last_token(hf(), attn, w, b)),
             "scores_from_hidden": (lambda: P.scores_mean_pooling_from_hidden(hid, mask, head), lambda: PO.scores_from_hidden(hf(), mask, w, b))}
    variants = [(f"{name}.{kind}", step(fn)) for name, fns in pairs.items() for kind, fn in zip(("kernel", "torch"), fns)]
    res = _rounds(variants, steps, warmup, rounds, dev)
    out = [dict(bench="pref_pool", variant=name, b=B, s=S, emb=E, hidden_bytes=B * S * E * 2, steps=steps, rounds=rounds, **r) for name, r in res.items()]
    out.append(dict(bench="pref_pool", variant="ratios", **{f"{name}_torch_over_kernel": res[f"{name}.torch"]["ms_median"] / res[f"{name}.kernel"]["ms_median"]
                                                            for name in pairs}))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--size", default="0.6B")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pool", type=int, nargs=3, default=(64, 512, 1024), help="(b, s, emb) of the pooling measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pref_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pref needs an MI355X")
    res = measure_pool(*a.pool, steps=4 * a.steps, warmup=a.warmup, rounds=a.rounds) + measure_dpo(a.pairs, a.seq, a.size, a.steps, a.warmup, a.rounds)
    for r in res:
        print(json.dumps(r))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
