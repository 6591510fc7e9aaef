"""Measure the GRPO loss paths on the GPU.

    python tools/bench_grpo.py [--batch 8] [--seq 512] [--vocab 151936] [--steps 20] [--warmup 5] [--rounds 3] [--out profiles/grpo_bench.json]

Qwen3-0.6B's head shape: ``batch x seq`` rows of ``vocab`` bf16 logits (8 x 512 x 151 936 = 1.24 GB).  Four variants alternate inside one process,
``--rounds`` times each, on the SAME buffer (refilled from a pristine copy outside the timed region, since three of them consume it):

  1. ``two_pass``: ``label_logprob_fwd``, the per-token chain, ``label_logprob_bwd`` in place -- reads the logits twice, writes them once;
  2. ``one_pass``: ``mi355_grpo_logits_loss`` in place -- reads once, writes once;
  3. ``forward``: ``label_logprob_fwd`` alone, what the old and the reference policy cost (twice per batch) -- reads once;
  4. ``cross_entropy``: the yardstick, ``mi355_cross_entropy`` with dlogits in place and ``ce_finalize`` -- moves the same bytes as (2).

Times are device events around whole calls, medians after warm-up, no profiler attached; a variant's figure is the median of its rounds' medians and every
round's median is kept (``round_ms_medians``) so the spread can be seen beside the differences.  Each is also given as achieved bytes / s (logits bytes
read + written, the [B, T] operands are noise) against the 6.3 TB/s a streaming copy achieves on this part (8 TB/s on paper).  Reported, not gated:
``one_pass / cross_entropy`` (expected within 15 %) and ``two_pass / one_pass`` (the feature's claim).  One JSON line per measurement on stdout, all of
them in ``--out``.  Needs the GPU.
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
HBM_ACHIEVABLE = 6.3e12  # bytes / s of a streaming copy (the microarchitecture notes' measured figure; 8.0e12 on paper)


def measure(B, S, V, steps, warmup, rounds):
    from llm_quest_amd import kernels as K0
    from llm_quest_amd import kernels_grpo as K

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    pristine = (3.0 * torch.randn(B, S, V, generator=g, device=dev)).to(BF16)
    work = torch.empty_like(pristine)
    ids = torch.randint(0, V, (B, S), generator=g, device=dev)
    T = S - 1
    work.copy_(pristine)
    logp, _ = K.label_logprob_fwd(work, ids)
    old = (logp + 0.3 * torch.randn(B, T, generator=g, device=dev)).contiguous()
    ref = (logp + 0.3 * torch.randn(B, T, generator=g, device=dev)).contiguous()
    adv = torch.randn(B, generator=g, device=dev)
    mask = torch.ones(B, T, dtype=torch.bool, device=dev)
    mask[:, : S // 4] = False
    targets = torch.cat([ids[:, 1:], torch.full((B, 1), -100, device=dev)], dim=1).reshape(-1).contiguous()
    args = (0.2, 0.2, 0.04, B, T, "grpo", False)

    def two_pass():
        lp, lse = K.label_logprob_fwd(work, ids)
        _, dlogp, _, _ = K.token_loss(lp, old, ref, adv, mask, *args)
        K.label_logprob_bwd(dlogp, work, lse, ids, out=work)

    def one_pass():
        K.logits_loss(work, ids, old, ref, adv, mask, *args, out=work)

    def forward():
        K.label_logprob_fwd(work, ids)

    flat = work.view(B * S, V)
    probe = torch.zeros(B * S, dtype=F32, device=dev)

    def cross_entropy():
        inv = K0.ce_finalize(probe, targets)[2:3]
        rows, _ = K0.cross_entropy(flat, targets, want_grad=True, grad_scale=inv, inplace=True)
        K0.ce_finalize(rows, targets)

    variants = (("two_pass", two_pass, 3), ("one_pass", one_pass, 2), ("forward", forward, 1), ("cross_entropy", cross_entropy, 2))
    runs = {name: [] for name, _, _ in variants}

    def timed(fn):  # the buffer is restored before every call, outside the events
        def run(steps_, warmup_):
            times = []
            for i in range(warmup_ + steps_):
                work.copy_(pristine)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                if i >= warmup_:
                    times.append(a.elapsed_time(b))
            times.sort()
            return {"ms_median": times[len(times) // 2], "ms_min": times[0], "ms_max": times[-1], "steps": steps_}

        return run

    for _ in range(rounds):
        for name, fn, _ in variants:
            runs[name].append(timed(fn)(steps, warmup))
    nbytes = B * S * V * 2
    out = []
    for name, _, passes in variants:
        meds = sorted(r["ms_median"] for r in runs[name])
        ms = meds[len(meds) // 2]
        moved = passes * nbytes
        out.append(dict(bench="grpo", variant=name, batch=B, seq=S, vocab=V, ms_median=ms, ms_min=min(r["ms_min"] for r in runs[name]),
                        ms_max=max(r["ms_max"] for r in runs[name]), round_ms_medians=[r["ms_median"] for r in runs[name]], steps=steps, rounds=rounds,
                        logits_bytes_moved=moved, bytes_per_s=moved / (ms * 1e-3), share_of_achievable_hbm=moved / (ms * 1e-3) / HBM_ACHIEVABLE))
    by = {o["variant"]: o["ms_median"] for o in out}
    out.append(dict(bench="grpo", variant="ratios", one_pass_over_cross_entropy=by["one_pass"] / by["cross_entropy"],
                    two_pass_over_one_pass=by["two_pass"] / by["one_pass"], hbm_achievable_bytes_per_s=HBM_ACHIEVABLE))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--vocab", type=int, default=151936)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grpo_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_grpo needs an MI355X")
    res = measure(a.batch, a.seq, a.vocab, a.steps, a.warmup, a.rounds)
    for r in res:
        print(json.dumps(r))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
