"""Measure the rollout path on the GPU: the row sampler against the torch-ops ``sampling``, and rollout tokens/s of ``generate_batched_rollouts`` against
``generate_batched_loop_kv_cache``.

    python tools/bench_rollout.py [--rows 64 256] [--vocab 151936] [--size 0.6B] [--batch 64] [--prompt 128] [--max-gen 64] [--steps 10] [--warmup 3] [--rounds 3]
                                  [--skip-model] [--out profiles/rollout_bench.json]

(i) The sampler alone on bf16 ``[rows, vocab]`` logits, 3 N(0, 1): ``top_k=20, temp=1``; ``top_p=0.9``; ``min_p=0.1``; ``top_p=0.9, top_k=20``.  ``sample_rows``
(explicit uniforms, so no generator work on either side's account) against ``generate.sampling`` on the same operand.  ``pass_fraction`` is the time one read
of the rows would take at the device's measured copy rate (a ``clone`` of the operand moves its bytes twice) over the sampler's time: 1 would be a sampler
that costs one pass.
(ii) Rollouts on Qwen3 ``--size`` with random weights, ``batch`` right-padded prompts of ``prompt`` tokens, ``max_gen`` new tokens, ``top_k=20, temp=1``, an EOS id
nothing samples (every row runs to ``max_gen``): ``generate_batched_rollouts`` at ``sync_every`` 1 and 8 against ``generate_batched_loop_kv_cache``.

The candidates alternate inside one process, ``--rounds`` times each; a figure is the median of its rounds' medians (device events around whole calls, after
warm-up, no profiler attached).  Reported, not gated.  One JSON line per measurement on stdout, all of them in ``--out``.  Needs the GPU.
"""

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))

from bench_deepseek_moe import time_calls  # noqa: E402

BF16 = torch.bfloat16
MODES = (("top_k20", {"top_k": 20}), ("top_p0.9", {"top_p": 0.9}), ("min_p0.1", {"min_p": 0.1}), ("top_p0.9_top_k20", {"top_p": 0.9, "top_k": 20}))


def alternate(variants, steps, warmup, rounds):
    runs = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            runs[name].append(time_calls(fn, steps, warmup)["ms_median"])
    return {name: dict(ms_median=sorted(r)[len(r) // 2], round_ms_medians=r) for name, r in runs.items()}


def measure_sampler(rows, vocab, steps, warmup, rounds, dev):
    from llm_quest_amd import generate as G

    g = torch.Generator(device=dev).manual_seed(0)
    x = (torch.randn(rows, vocab, generator=g, device=dev) * 3).to(BF16)
    u = torch.rand(rows, generator=g, device=dev)
    copy = alternate([("clone", lambda: x.clone())], steps, warmup, rounds)["clone"]["ms_median"]
    one_pass_ms = copy / 2
    out = []
    for name, kw in MODES:
        res = alternate([("sample_rows", lambda: G.sample_rows(x, temp=1.0, uniforms=u, **kw)), ("torch_sampling", lambda: G.sampling(x, temp=1.0, **kw))],
                        steps, warmup, rounds)
        out.append(dict(kind="sampler", rows=rows, vocab=vocab, mode=name, sample_rows_ms=res["sample_rows"]["ms_median"],
                        torch_sampling_ms=res["torch_sampling"]["ms_median"], speedup=res["torch_sampling"]["ms_median"] / res["sample_rows"]["ms_median"],
                        one_pass_ms=one_pass_ms, pass_fraction=one_pass_ms / res["sample_rows"]["ms_median"], rounds=res))
    return out


def measure_rollouts(size, batch, prompt, max_gen, steps, warmup, rounds, dev):
    from llm_quest_amd import generate as G
    from llm_quest_amd.config import qwen3_config_creator
    from llm_quest_amd.qwen.qwen3.qwen3_model import Qwen3Model

    cfg = qwen3_config_creator(size)
    cfg["context_length"] = prompt + max_gen
    torch.manual_seed(0)
    model = Qwen3Model(cfg).to(dev).eval()
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, cfg["vocab_size"] - 1, (batch, prompt), generator=g).to(dev)
    lens = torch.randint(prompt // 2, prompt + 1, (batch,), generator=g)
    mask = (torch.arange(prompt)[None, :] < lens[:, None]).to(dev)
    eos = cfg["vocab_size"] - 1  # never in the prompts; a sampled one would only shorten both candidates alike
    common = dict(top_k=20, temp=1.0, eos_ids=eos, pad_id=eos, device=dev, attention_mask=mask)
    rng = G.SampleRNG(0)
    variants = [("rollouts_sync1", lambda: G.generate_batched_rollouts(ids, model, max_gen, cfg["context_length"], rng=rng, sync_every=1, **common)),
                ("rollouts_sync8", lambda: G.generate_batched_rollouts(ids, model, max_gen, cfg["context_length"], rng=rng, sync_every=8, **common)),
                ("torch_loop", lambda: G.generate_batched_loop_kv_cache(ids, model, max_gen, cfg["context_length"], **common))]
    res = alternate(variants, steps, warmup, rounds)
    tok = lambda name: batch * max_gen / (res[name]["ms_median"] * 1e-3)
    return dict(kind="rollouts", size=size, batch=batch, prompt=prompt, max_gen=max_gen, tokens_per_s={n: tok(n) for n, _ in variants},
                speedup_sync1=res["torch_loop"]["ms_median"] / res["rollouts_sync1"]["ms_median"],
                speedup_sync8=res["torch_loop"]["ms_median"] / res["rollouts_sync8"]["ms_median"], rounds=res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--vocab", type=int, default=151936)
    ap.add_argument("--size", default="0.6B")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--max-gen", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout needs an MI355X")
    dev = torch.device("cuda", 0)
    results = []
    for rows in a.rows:
        results += measure_sampler(rows, a.vocab, a.steps, a.warmup, a.rounds, dev)
    if not a.skip_model:
        results.append(measure_rollouts(a.size, a.batch, a.prompt, a.max_gen, max(a.steps // 3, 2), 1, a.rounds, dev))
    for r in results:
        print(json.dumps(r))
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
