"""Measure one Qwen3 mixture-of-experts layer on the GPU.

    python tools/bench_moe.py [--tokens 4096] [--steps 20] [--warmup 5] [--out profiles/moe_bench.json]

Subject: one ``Qwen3MoE`` layer, forward + backward, at the ``temp_moe`` shape (d = 896, F = 3584, E = 16, k = 4) on T = 4096 tokens, routed by
a trained-like gate (gate weights scaled so that the probabilities are peaked; random tokens).  On the same box, in the same process:
  * the whole layer (``ops_moe.MoEFn``), device events around forward + backward, with ``ops_moe.SEGMENTED`` on (segmented GEMMs: one launch per product
    over all experts, no host read) and off (per-expert launches behind the read of the counts): both medians and their ratio, from this one run;
  * its split: the row kernels of csrc/moe.hip alone (route, column sums, plan, gather, combine, their backwards), the expert GEMMs alone (forward + backward
    with the weight gradients on prepared segments: the layer's own per-expert loops of ``ops_moe``, all forwards then all backwards, and the six
    segmented launches), the gate's three GEMMs, and the host's
    wait on the ``E`` counts (host clock around the one device-to-host read, queue drained before the router is enqueued);
  * the dense SwiGLU FFN of the same activated width (hidden = k * F) through the existing kernels, forward + backward;
  * one ``30B-A3B``-shaped layer (d = 2048, F = 768, E = 128, k = 8), both paths: what 128 experts' launches cost.
Medians after warm-up, no profiler attached; one JSON line per measurement on stdout, all of them in ``--out``.  No threshold: the comparison is the
other path in the same run.  Needs the GPU.
"""

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16, F32 = torch.bfloat16, torch.float32


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def time_calls(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return {"ms_median": median(times), "ms_min": min(times), "ms_max": max(times), "steps": steps}


def build_layer(d, F_, E, k, T, seed=0):
    from llm_quest_amd.moe.qwen3_moe import Qwen3MoE

    torch.manual_seed(seed)
    moe = Qwen3MoE(dict(emb_dim=d, moe_hidden_dim=F_, num_experts=E, top_k=k, aux_loss_coef=0.001, dtype=BF16)).cuda().train()
    with torch.no_grad():
        moe.gate.weight.mul_(8.0)  # a trained gate is peaked; a fresh one is near uniform
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(1, T, d, generator=g).to(BF16).cuda()
    dy = torch.randn(1, T, d, generator=g).to(BF16).cuda()
    return moe, x, dy


def measure_layer(name, d, F_, E, k, T, steps, warmup, split):
    from llm_quest_amd import _lib as L
    from llm_quest_amd import kernels as K
    from llm_quest_amd import kernels_moe as KM
    from llm_quest_amd import ops, ops_moe

    moe, x, dy = build_layer(d, F_, E, k, T)
    one = torch.ones((), dtype=BF16, device="cuda")

    def whole():
        xg = x.detach().requires_grad_(True)
        out = moe(xg)
        torch.autograd.backward([out, moe.moe_loss], [dy, one])
        return xg.grad

    # the layer with the switch on (segmented GEMMs: no host read, one launch per product) and off (per-expert launches behind the read of the counts),
    # same process, same tensors, the shipped default last so that everything below runs on it
    default, by_switch = ops_moe.SEGMENTED, {}
    for on in (not default, default):
        ops_moe.SEGMENTED = on
        whole()
        by_switch[on] = time_calls(whole, steps, warmup)
    r = by_switch[default]
    arena = ops.arena_for(moe)
    h = x[0]
    logits = K.gemm(L.GEMM_NT, h, moe.gate.weight)
    p, idx, w, s = KM.route_fwd(logits, k)
    counts, offsets, slot, row_token, _ = KM.plan(idx, E, K.colsum(p), 0.001)
    n_rows = counts.tolist()
    hit = sum(1 for n in n_rows if n)
    res = dict(kind="layer", name=name, d=d, F=F_, E=E, k=k, T=T, fwd_bwd_ms=r["ms_median"], fwd_bwd_ms_min=r["ms_min"], fwd_bwd_ms_max=r["ms_max"], steps=steps,
               experts_hit=hit, rows_min=min(n_rows), rows_max=max(n_rows),
               default_path="segmented" if default else "per-expert",
               segmented_fwd_bwd_ms=by_switch[True]["ms_median"], segmented_fwd_bwd_ms_min=by_switch[True]["ms_min"], segmented_fwd_bwd_ms_max=by_switch[True]["ms_max"],
               per_expert_fwd_bwd_ms=by_switch[False]["ms_median"], per_expert_fwd_bwd_ms_min=by_switch[False]["ms_min"], per_expert_fwd_bwd_ms_max=by_switch[False]["ms_max"],
               per_expert_over_segmented=by_switch[False]["ms_median"] / by_switch[True]["ms_median"],
               launches=dict(segmented=dict(expert_gemms_fwd=2, expert_gemms_bwd=2, weight_gradient_launches=2, gate_weight_gradient_launches=1, row_kernels=10, gate_gemms=3),
                             per_expert=dict(expert_gemms_fwd=2 * hit, expert_gemms_bwd=2 * hit, weight_gradient_problems=2 * hit + 1,
                                             grouped_weight_gradient_launches=(2 * hit + 1 + 7) // 8, row_kernels=10, gate_gemms=3)))
    if not split:
        return [res]
    out = [res]
    # ---- the row kernels alone, on the layer's own tensors
    xs = KM.gather_rows(h, row_token)
    y = torch.randn(xs.shape, generator=torch.Generator().manual_seed(5)).to(BF16).cuda()
    g1 = torch.ones(1, dtype=F32, device="cuda")

    def rows():
        p_, idx_, w_, s_ = KM.route_fwd(logits, k)
        c_, _, slot_, rt_, _ = KM.plan(idx_, E, K.colsum(p_), 0.001)
        xs_ = KM.gather_rows(h, rt_)
        KM.combine_fwd(y, slot_, w_, h)
        dy_, dw_ = KM.combine_bwd(dy[0], rt_, slot_, w_, y)
        KM.combine_fwd(dy_, slot_)
        KM.route_bwd(dw_, w_, s_, idx_, p_, c_, g1, 0.001)

    out.append(dict(kind="split", name=name, part="row kernels (route, colsum, plan, gather, combine, combine backward, gather backward, route backward)",
                    **time_calls(rows, steps, warmup)))
    # ---- the expert GEMMs alone: the layer's own per-expert loops (ops_moe) on the counts read above, all forwards, then all backwards with the weight gradients
    def experts():
        wg = []
        _, gus, acts, segs = ops_moe._experts_forward_loop(moe.experts, "lin1", "lin_gate", arena, xs, n_rows, F_)
        ops_moe._experts_backward_loop(moe.experts, "lin1", "lin_gate", arena, xs, gus, acts, segs, y, F_, wg)
        ops._flush_wgrads(wg)

    out.append(dict(kind="split", name=name, part="expert GEMMs, per-expert launches (gate-up + SwiGLU, lin2, their dgrads, grouped weight gradients)",
                    **time_calls(experts, steps, warmup)))
    st = ops_moe.expert_stacks(moe, arena, moe.experts, "lin1", "lin_gate")

    def experts_segmented():
        gu, a, _ = ops_moe.experts_forward(st, xs, counts, offsets, T * k, F_)
        ops_moe.experts_backward(st, arena, xs, gu, a, y, counts, offsets, T * k, F_)

    out.append(dict(kind="split", name=name, part="expert GEMMs, segmented (the same six products, one launch each over all experts, no host read)",
                    **time_calls(experts_segmented, steps, warmup)))
    dlogits = torch.randn(logits.shape, generator=torch.Generator().manual_seed(6)).to(BF16).cuda()
    dh = torch.zeros_like(h)

    def gate():
        wg = []
        K.gemm(L.GEMM_NT, h, moe.gate.weight)
        K.gemm(L.GEMM_NN, dlogits, moe.gate.weight, out=dh, residual=dh)
        ops._wgrad(arena, moe.gate.weight, None, dlogits, h, wg)
        ops._flush_wgrads(wg)

    out.append(dict(kind="split", name=name, part="gate GEMMs (logits, dgrad, weight gradient)", **time_calls(gate, steps, warmup)))
    # ---- the host's wait on the counts: queue drained, the layer's front enqueued, then the one device-to-host read
    waits, fronts = [], []
    for i in range(steps + warmup):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lg = K.gemm(L.GEMM_NT, h, moe.gate.weight)
        p_, idx_, _, _ = KM.route_fwd(lg, k)
        c_ = KM.plan(idx_, E, K.colsum(p_), 0.001)[0]
        t1 = time.perf_counter()
        c_.tolist()
        t2 = time.perf_counter()
        if i >= warmup:
            fronts.append((t1 - t0) * 1e3)
            waits.append((t2 - t1) * 1e3)
    out.append(dict(kind="split", name=name, part="host: enqueue of the gate GEMM, router, column sums and plan, then the wait inside the read of the counts",
                    enqueue_ms_median=median(fronts), host_wait_ms_median=median(waits), host_wait_ms_min=min(waits), host_wait_ms_max=max(waits), steps=steps))
    return out


def measure_dense(d, hidden, T, steps, warmup):
    from llm_quest_amd.qwen.qwen3.qwen3_transformer_block import FFN

    torch.manual_seed(0)
    ffn = FFN(dict(emb_dim=d, hidden_dim=hidden, dtype=BF16)).cuda().train()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, T, d, generator=g).to(BF16).cuda()
    dy = torch.randn(1, T, d, generator=g).to(BF16).cuda()

    def step():
        xg = x.detach().requires_grad_(True)
        ffn(xg).backward(dy)
        return xg.grad

    step()
    r = time_calls(step, steps, warmup)
    return dict(kind="dense", name=f"dense SwiGLU FFN of the activated width (hidden = {hidden})", d=d, hidden=hidden, T=T, fwd_bwd_ms=r["ms_median"],
                fwd_bwd_ms_min=r["ms_min"], fwd_bwd_ms_max=r["ms_max"], steps=steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moe_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_moe.py needs an MI355X: there is nothing to measure without one")
    results = []

    def emit(r):
        results.append(r)
        print(json.dumps(r), flush=True)

    T = args.tokens
    for r in measure_layer("temp_moe", 896, 3584, 16, 4, T, args.steps, args.warmup, split=True):
        emit(r)
    emit(measure_dense(896, 4 * 3584, T, args.steps, args.warmup))
    for r in measure_layer("30B-A3B", 2048, 768, 128, 8, T, args.steps, args.warmup, split=False):
        emit(r)
    emit(measure_dense(2048, 8 * 768, T, args.steps, args.warmup))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(note="tools/bench_moe.py: one Qwen3MoE layer forward + backward, its split, the dense FFN of the same activated width; device-event "
                                "times (host clock for the wait on the counts), no profiler", torch=torch.__version__, device=torch.cuda.get_device_name(0),
                           results=results), f, indent=1)


if __name__ == "__main__":
    main()
