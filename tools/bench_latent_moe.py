"""Measure the LatentMoE path on the GPU.

    python tools/bench_latent_moe.py [--tokens 4096] [--steps 20] [--warmup 5] [--rounds 3] [--out profiles/latent_moe_bench.json]

One ``LatentMoE`` layer at the upstream defaults (``latent_ratio`` 4: 16 routed experts, top_k 8, at the latent width 192) on the ``emb_dim`` and hidden
size ``bench_deepseek_moe.py`` uses (768 and 768), forward + backward on ``--tokens`` tokens, in ONE run beside
  * the same layer on the per-expert path (``ops_moe.SEGMENTED`` off: one host read of the counts, launches per expert), and
  * a ``DeepSeekMoE`` of the same ``emb_dim`` with a quarter of the routed experts (4) and of the top_k (2) at full width and one shared expert: the
    layer the Nemotron-3 paper says costs the same,
and the layer's time spent in what ``csrc/latent_moe.hip`` adds: the two squared-ReLU GLU passes (routed experts over the whole sorted buffer, shared
expert; forward + backward each) and the two router kernels.  That share is what fusing the activation into the gate-up write-out could win at most.

The three whole-layer variants alternate inside the process, ``--rounds`` times each; a variant's figure is the median of its rounds' medians, and every
round's median is kept (``round_ms_medians``) so the spread can be seen beside the differences.  Times are device events around whole calls, medians
after warm-up, no profiler attached; one JSON line per measurement on stdout, all of them in
``--out``.  Nothing is gated: the numbers are DESIGN.md section 5.  Needs the GPU.
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
EMB, HIDDEN = 768, 768  # DEEPSEEK_SMALL_CONFIG's emb_dim and scaled hidden size


def _step_of(moe, x, dy):
    def step():
        for p in moe.parameters():
            p.grad = None
        x.grad = None
        moe(x).backward(dy)

    return step


def measure(T, steps, warmup, rounds):
    from llm_quest_amd import kernels_latmoe as KL
    from llm_quest_amd import kernels_moe as KM
    from llm_quest_amd import ops_moe
    from llm_quest_amd.moe.deepseek_moe import DeepSeekMoE
    from llm_quest_amd.moe.nvidia_latent_moe import LatentMoE

    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, T, EMB, generator=g).to(BF16).cuda().requires_grad_(True)
    dy = torch.randn(1, T, EMB, generator=g).to(BF16).cuda()
    torch.manual_seed(0)
    moe = LatentMoE(dict(emb_dim=EMB, moe_hidden_dim=HIDDEN, dtype=BF16)).to(BF16).cuda().train()
    E, k, lat, F_ = moe.num_experts, moe.top_k, moe.latent_dim, moe.routed_experts[0].hidden_dim
    step = _step_of(moe, x, dy)
    # the layer the paper equates it with: a quarter of the experts and of the top_k at full width, one shared expert
    torch.manual_seed(0)
    ds = DeepSeekMoE(dict(emb_dim=EMB, hidden_dim=HIDDEN, dtype=BF16, num_experts=E // 4 + 1, num_shared_experts=1, top_k=k // 4, moe_scaling_factor=1,
                          moe_bias_update_rate=1e-3)).to(BF16).cuda().train()
    ds_step = _step_of(ds, x, dy)

    default = ops_moe.SEGMENTED
    runs = {"segmented": [], "per_expert": [], "full_width": []}
    for _ in range(rounds):  # the variants alternate; the shipped default of the switch is restored behind every round
        for name, on, fn in (("per_expert", False, step), ("segmented", True, step), ("full_width", default, ds_step)):
            ops_moe.SEGMENTED = on
            fn()
            runs[name].append(time_calls(fn, steps, warmup))
        ops_moe.SEGMENTED = default

    def fold(rs):
        meds = sorted(r["ms_median"] for r in rs)
        return dict(ms_median=meds[len(meds) // 2], ms_min=min(r["ms_min"] for r in rs), ms_max=max(r["ms_max"] for r in rs), steps=steps, rounds=len(rs),
                    round_ms_medians=[r["ms_median"] for r in rs])

    seg, per, full = fold(runs["segmented"]), fold(runs["per_expert"]), fold(runs["full_width"])
    counts = moe._routed[1]
    layer = dict(kind="layer", name=f"LatentMoE forward + backward (emb {EMB}, latent {lat}, {E} routed experts of hidden {F_}, top_k {k}, 1 shared expert of hidden {F_})",
                 tokens=T, counts=counts.tolist(), default_path="segmented" if default else "per-expert",
                 segmented_ms_median=seg["ms_median"], segmented_round_ms_medians=seg["round_ms_medians"],
                 per_expert_ms_median=per["ms_median"], per_expert_round_ms_medians=per["round_ms_medians"],
                 per_expert_over_segmented=per["ms_median"] / seg["ms_median"], **(seg if default else per))
    out = [layer]
    out.append(dict(kind="layer", name=f"DeepSeekMoE forward + backward (emb {EMB}, {E // 4} routed experts of hidden {HIDDEN} at full width, top_k {k // 4}, 1 shared expert)",
                    tokens=T, latent_over_full_width=layer["ms_median"] / full["ms_median"], **full))

    # what csrc/latent_moe.hip adds, on the layer's own shapes
    R = KM.sorted_rows(T, E, k)
    gu_r = torch.randn(R, 2 * F_, generator=g).to(BF16).cuda()
    da_r = torch.randn(R, F_, generator=g).to(BF16).cuda()
    Fs = moe.shared_expert.hidden_dim
    gu_s = torch.randn(T, 2 * Fs, generator=g).to(BF16).cuda()
    da_s = torch.randn(T, Fs, generator=g).to(BF16).cuda()
    logits = torch.randn(T, E, generator=g).to(BF16).cuda()
    dw = torch.randn(T, k, generator=g).cuda()
    p, idx, w, s = KL.route_fwd(logits, moe.biases, k, 2.5)

    def activation():
        KL.relu2_glu_fwd(gu_r, F_)
        KL.relu2_glu_bwd(gu_r, da_r, F_)
        KL.relu2_glu_fwd(gu_s, Fs)
        KL.relu2_glu_bwd(gu_s, da_s, Fs)

    def router():
        KL.route_fwd(logits, moe.biases, k, 2.5)
        KL.route_bwd(dw, s, idx, p, 2.5)

    for name, fn in ((f"squared-ReLU GLU, forward + backward: routed experts ([{R}, {2 * F_}] sorted rows) and shared expert ([{T}, {2 * Fs}])", activation),
                     ("sigmoid router, forward + backward kernels", router)):
        r = time_calls(fn, steps, warmup)
        out.append(dict(kind="part", name=name, tokens=T, share_of_layer=r["ms_median"] / layer["ms_median"], **r))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "latent_moe_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_latent_moe.py needs an MI355X: there is nothing to measure without one")
    results = []
    for r in measure(args.tokens, args.steps, args.warmup, args.rounds):
        results.append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(note="tools/bench_latent_moe.py: one LatentMoE layer forward + backward at the upstream defaults on both expert paths, the DeepSeekMoE layer "
                                "with a quarter of the experts and of the top_k at full width, and the layer's squared-ReLU GLU and router kernels on their own; "
                                "device-event times, no profiler",
                           torch=torch.__version__, device=torch.cuda.get_device_name(0), results=results), f, indent=1)


if __name__ == "__main__":
    main()
