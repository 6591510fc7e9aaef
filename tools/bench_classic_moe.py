"""Measure the classic MoE path on the GPU.

    python tools/bench_classic_moe.py [--tokens 4096] [--steps 20] [--warmup 5] [--rounds 3] [--out profiles/classic_moe_bench.json]

One ``MoE`` layer at ``emb_dim`` 768 with the upstream defaults (8 experts, top-2, "auto": hidden 1 536), forward + backward on ``--tokens`` tokens with the
loss in the backward, in ONE run beside
  * the same layer on the per-expert path (``ops_moe.SEGMENTED`` off: one host read of the counts, one GEMM per expert and product), and
  * the dense GPT-2 FFN of the same activated width (``ExpertGeLU`` on its own at scaling factor 1: 768 -> 3 072 -> 768, bias and erf GELU through the
    GEMM's epilogues),
and the layer's time spent in the row kernels this layer brought: the router (forward, loss, backward), bias + GELU, the second bias, the GELU backward
and the two per-segment column sums, each on the layer's own shapes.  The bias and GELU passes' share is what a per-expert-bias epilogue of the segmented
GEMM could win at most.

The three whole-layer variants alternate inside the process, ``--rounds`` times each; a variant's figure is the median of its rounds' medians, and every
round's median is kept (``round_ms_medians``) so the spread can be seen beside the differences.  Times are device events around whole calls, medians
after warm-up, no profiler attached; one JSON line per measurement on stdout, all of them in ``--out``.  Nothing is gated: the numbers are DESIGN.md
section 5.  Needs the GPU.
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
EMB = 768


def measure(T, steps, warmup, rounds):
    from llm_quest_amd import kernels as K
    from llm_quest_amd import kernels_cmoe as KC
    from llm_quest_amd import kernels_moe as KM
    from llm_quest_amd import ops_cmoe, ops_moe
    from llm_quest_amd.moe.classic_moe import ExpertGeLU, MoE

    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, T, EMB, generator=g).to(BF16).cuda().requires_grad_(True)
    dy = torch.randn(1, T, EMB, generator=g).to(BF16).cuda()
    one = torch.ones((), dtype=BF16, device="cuda")
    torch.manual_seed(0)
    moe = MoE(dict(emb_dim=EMB)).to(BF16).cuda().train()
    E, k, H = moe.num_experts, moe.top_k, moe.experts[0].hidden_dim
    torch.manual_seed(0)
    ffn = ExpertGeLU(dict(emb_dim=EMB), 1.0).to(BF16).cuda().train()

    def step():
        for p in moe.parameters():
            p.grad = None
        x.grad = None
        out = moe(x)
        torch.autograd.backward([out, moe.moe_loss], [dy, one])

    def dense_step():
        for p in ffn.parameters():
            p.grad = None
        x.grad = None
        ffn(x).backward(dy)

    default = ops_moe.SEGMENTED
    runs = {"segmented": [], "per_expert": [], "dense": []}
    for _ in range(rounds):  # the variants alternate; the shipped default of the switch is restored behind every round
        for name, on, fn in (("per_expert", False, step), ("segmented", True, step), ("dense", default, dense_step)):
            ops_moe.SEGMENTED = on
            fn()
            runs[name].append(time_calls(fn, steps, warmup))
        ops_moe.SEGMENTED = default

    def fold(rs):
        meds = sorted(r["ms_median"] for r in rs)
        return dict(ms_median=meds[len(meds) // 2], ms_min=min(r["ms_min"] for r in rs), ms_max=max(r["ms_max"] for r in rs), steps=steps, rounds=len(rs),
                    round_ms_medians=[r["ms_median"] for r in rs])

    seg, per, dense = fold(runs["segmented"]), fold(runs["per_expert"]), fold(runs["dense"])
    counts, offsets = moe._routed[1], None
    layer = dict(kind="layer", name=f"classic MoE forward + backward (emb {EMB}, {E} experts of hidden {H}, top_k {k}, loss in the backward)",
                 tokens=T, counts=counts.tolist(), default_path="segmented" if default else "per-expert",
                 segmented_ms_median=seg["ms_median"], segmented_round_ms_medians=seg["round_ms_medians"],
                 per_expert_ms_median=per["ms_median"], per_expert_round_ms_medians=per["round_ms_medians"],
                 per_expert_over_segmented=per["ms_median"] / seg["ms_median"], **(seg if default else per))
    out = [layer]
    out.append(dict(kind="layer", name=f"dense GPT-2 FFN forward + backward (ExpertGeLU alone: {EMB} -> {4 * EMB} -> {EMB}, bias and erf GELU in the GEMM's epilogues)",
                    tokens=T, moe_over_dense=layer["ms_median"] / dense["ms_median"], **dense))

    # the row kernels this layer brought, on the layer's own shapes and on a routing of its own
    logits = torch.randn(T, E, generator=g).to(BF16).cuda()
    dw = torch.randn(T, k, generator=g).cuda()
    gl = torch.ones(1, dtype=F32, device="cuda")
    p, idx, w, s, lse = KC.route_fwd(logits, k)
    counts, offsets, slot, row_token, load = KM.plan(idx, E, K.colsum(p), moe.load_coeff)
    R = row_token.numel()
    st = ops_cmoe.expert_stacks(moe, moe._arena)
    zh = torch.randn(R, H, generator=g).to(BF16).cuda()
    dh = torch.randn(R, H, generator=g).to(BF16).cuda()
    zd = torch.randn(R, EMB, generator=g).to(BF16).cuda()
    act = torch.empty_like(zh)
    pre = torch.empty_like(zh)
    yd = torch.empty_like(zd)
    gb1 = torch.empty((E, 1, H), dtype=BF16, device="cuda")
    gb2 = torch.empty((E, 1, EMB), dtype=BF16, device="cuda")

    def router():
        KC.route_fwd(logits, k)
        KC.loss(lse, moe.z_router_coeff, load)
        KC.route_bwd(dw, w, s, idx, p, counts, gl, moe.load_coeff, moe.z_router_coeff, lse)

    parts = ((f"router: forward, loss and backward kernels ([{T}, {E}])", router),
             (f"bias + GELU over the sorted rows ([{R}, {H}])", lambda: KC.bias_act_fwd(zh, st.b1, counts, offsets, gelu=True, pre=pre, act=act)),
             (f"second bias over the sorted rows ([{R}, {EMB}])", lambda: KC.bias_act_fwd(zd, st.b2, counts, offsets, gelu=False, pre=yd)),
             (f"GELU backward over the sorted rows ([{R}, {H}])", lambda: KC.gelu_bwd(zh, dh)),
             (f"per-segment column sums: both bias gradients ([{R}, {H}] and [{R}, {EMB}])",
              lambda: (KC.segment_colsum(dh, counts, offsets, gb1), KC.segment_colsum(zd, counts, offsets, gb2))))
    total = 0.0
    for name, fn in parts:
        r = time_calls(fn, steps, warmup)
        total += r["ms_median"]
        out.append(dict(kind="part", name=name, tokens=T, share_of_layer=r["ms_median"] / layer["ms_median"], **r))
    out.append(dict(kind="sum", name="all row kernels of csrc/classic_moe.hip and the GELU backward, timed one by one", tokens=T, ms_median=total,
                    share_of_layer=total / layer["ms_median"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classic_moe_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_classic_moe.py needs an MI355X: there is nothing to measure without one")
    results = []
    for r in measure(args.tokens, args.steps, args.warmup, args.rounds):
        results.append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(note="tools/bench_classic_moe.py: one classic MoE layer forward + backward (emb 768, 8 experts, top-2, hidden 1536) on both expert paths, the "
                                "dense GPT-2 FFN of the same activated width, and the layer's row kernels on their own; device-event times, no profiler",
                           torch=torch.__version__, device=torch.cuda.get_device_name(0), results=results), f, indent=1)


if __name__ == "__main__":
    main()
