"""Measure the GRPO loss from hidden states (vocabulary-chunked LM head) against the loss on materialised logits, on the GPU.

    python tools/bench_grpo_head.py [--batch 8] [--seq 512] [--emb 1024] [--vocab 151936] [--steps 10] [--warmup 3] [--rounds 3]
                                    [--chunks W ...] [--out profiles/grpo_head_bench.json]

Qwen3-0.6B's head: ``batch x seq`` hidden rows of ``emb`` against a ``vocab x emb`` weight (8 x 512 x 151 936 logits = 1.24 GB when they exist).  The variants
alternate inside one process, ``--rounds`` times each, through the public functions and autograd, on the same operands:

  a. ``materialised``: ``out_head(hidden)``, ``grpo_policy_loss`` (one pass, in place), ``backward()`` (the head's dgrad and weight-gradient GEMMs);
  b. ``chunked`` at the default ``vocab_chunk`` (``kernels_grpo_head.head_chunks``) and at half and double of it: ``grpo_policy_loss_from_hidden`` and
     ``backward()`` -- 4 / 3 of (a)'s GEMM work by construction, none of its logits;
  c. the no-grad forward of one policy (the old and the reference policy cost it once each per batch): ``forward_chunked`` =
     ``log_probs_per_token_from_hidden``, the head part of ``Qwen3Model.label_log_probs``, against ``forward_materialised`` = ``out_head(hidden)`` +
     ``log_probs_per_token`` (the ``forward_hidden`` in front is the same in both and is not run).

Times are device events around whole calls, medians after warm-up, no profiler attached; a variant's figure is the median of its rounds' medians and every
round's median is kept (``round_ms_medians``).  ``peak_bytes`` is the rise of ``torch.cuda.max_memory_allocated`` over one call above the level in front of
it (operands, the weight's gradient and the GEMMs' split-K workspace already allocated).  Reported, not gated: ``chunked / materialised`` per chunk width and
which width won.  One JSON line per measurement on stdout, all of them in ``--out``.  Needs the GPU.
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

BF16, F32 = torch.bfloat16, torch.float32


def head_flops(rows, D, V, products):
    return 2 * rows * D * V * products


def measure(B, S, D, V, steps, warmup, rounds, chunks=None):
    from llm_quest_amd import kernels_grpo_head as KH
    from llm_quest_amd.alignment.rlhf_grpo import grpo_engine as G
    from llm_quest_amd.qwen.qwen3.qwen3_model import _OutHead

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    head = _OutHead(torch.nn.Parameter((torch.randn(V, D, generator=g, device=dev) / D ** 0.5).to(BF16)))
    hid = torch.randn(B, S, D, generator=g, device=dev).to(BF16).requires_grad_(True)
    ids = torch.randint(0, V, (B, S), generator=g, device=dev)
    T = S - 1
    with torch.no_grad():
        logp = G.log_probs_per_token_from_hidden(hid, head, ids)
    old = (logp + 0.3 * torch.randn(B, T, generator=g, device=dev)).contiguous()
    ref = (logp + 0.3 * torch.randn(B, T, generator=g, device=dev)).contiguous()
    adv = torch.randn(B, generator=g, device=dev)
    mask = torch.ones(B, T, dtype=torch.bool, device=dev)
    mask[:, : S // 4] = False
    kw = dict(num_samples=B, min_clip=0.2, max_clip=0.2, beta=0.04, max_gen=T)
    default = KH.head_chunks(B * S, V)[0][1]

    def materialised():
        hid.grad = None
        G.grpo_policy_loss(head(hid), ids, old, ref, adv, mask, **kw).backward()

    def chunked(step):
        def run():
            hid.grad = None
            G.grpo_policy_loss_from_hidden(hid, head, ids, old, ref, adv, mask, vocab_chunk=step, **kw).backward()

        return run

    def forward_materialised():
        with torch.no_grad():
            G.log_probs_per_token(head(hid), ids)

    def forward_chunked():
        with torch.no_grad():
            G.log_probs_per_token_from_hidden(hid, head, ids)

    widths = sorted(set(chunks)) if chunks else sorted({max(128, default // 2 // 128 * 128), default, min(default * 2, (V + 7) // 8 * 8)})
    variants = [("materialised", materialised, 3, None)] + [(f"chunked_{w}", chunked(w), 4, w) for w in widths]
    variants += [("forward_materialised", forward_materialised, 1, None), ("forward_chunked", forward_chunked, 1, default)]
    runs = {name: [] for name, *_ in variants}
    for _ in range(rounds):
        for name, fn, _, _ in variants:
            runs[name].append(time_calls(fn, steps, warmup))
    peaks = {}
    for name, fn, _, _ in variants:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        fn()
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated(dev) - base
    out = []
    for name, _, products, width in variants:
        meds = sorted(r["ms_median"] for r in runs[name])
        ms = meds[len(meds) // 2]
        flops = head_flops(B * S, D, V, products)
        out.append(dict(bench="grpo_head", variant=name, batch=B, seq=S, emb=D, vocab=V, vocab_chunk=width, ms_median=ms,
                        ms_min=min(r["ms_min"] for r in runs[name]), ms_max=max(r["ms_max"] for r in runs[name]),
                        round_ms_medians=[r["ms_median"] for r in runs[name]], steps=steps, rounds=rounds, head_gemm_products=products, head_gemm_flops=flops,
                        head_gemm_flops_per_s=flops / (ms * 1e-3), peak_bytes=peaks[name]))
    by = {o["variant"]: o["ms_median"] for o in out}
    ratios = {f"chunked_{w}_over_materialised": by[f"chunked_{w}"] / by["materialised"] for w in widths}
    best = min(widths, key=lambda w: by[f"chunked_{w}"])
    out.append(dict(bench="grpo_head", variant="ratios", default_vocab_chunk=default, best_vocab_chunk=best, logits_bytes=B * S * V * 2,
                    forward_chunked_over_materialised=by["forward_chunked"] / by["forward_materialised"], **ratios))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--emb", type=int, default=1024)
    ap.add_argument("--vocab", type=int, default=151936)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunks", type=int, nargs="*", default=None, help="vocab_chunk widths of variant (b) instead of half / default / double")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grpo_head_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_grpo_head needs an MI355X")
    res = measure(a.batch, a.seq, a.emb, a.vocab, a.steps, a.warmup, a.rounds, a.chunks)
    for r in res:
        print(json.dumps(r))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
