"""Measure the DeepSeekMoE path on the GPU.

    python tools/bench_deepseek_moe.py [--tokens 4096] [--steps 20] [--warmup 5] [--out profiles/deepseek_moe_bench.json]

One DeepSeekMoE layer of ``DEEPSEEK_SMALL_CONFIG`` (emb 768, 7 routed + 1 shared expert of hidden 768, top_k 3), forward + backward on
``--tokens`` tokens, and its split as ``bench_moe.py`` splits: router and bias update (gate GEMM, route forward / backward, the update), plan,
rows (dispatch, combine and their backwards), shared experts, routed expert GEMMs (the layer's own per-expert loops of ``ops_moe`` on the layer's own
counts, the host read included, all forwards then all backwards, and the six segmented launches).  The layer and the model steps run with ``ops_moe.SEGMENTED`` on and off in this one process: both medians
and their ratio are in the output.  The dense ``FFN`` of the same config (hidden 3072) on the same tokens in the same run.  Then the training step of
``DEEPSEEK_SMALL_CONFIG`` as written (3 dense + 9 MoE blocks, mtp_depth 2) beside the all-dense one ``bench_deepseek.py`` measures.

Times are device events around whole calls, medians after warm-up, no profiler attached; one JSON line per measurement on stdout, all of them
in ``--out``.  Nothing is gated: the numbers and what bounds them are DESIGN.md section 5.  Needs the GPU.
"""

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))

BF16, F32 = torch.bfloat16, torch.float32


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
    times.sort()
    return {"ms_median": times[len(times) // 2], "ms_min": times[0], "ms_max": times[-1], "steps": steps}


def measure_layer(cfg, T, steps, warmup):
    from llm_quest_amd import _lib as L
    from llm_quest_amd import kernels as K
    from llm_quest_amd import kernels_dsmoe as KD
    from llm_quest_amd import kernels_moe as KM
    from llm_quest_amd import ops_dsmoe, ops_moe
    from llm_quest_amd.moe.deepseek_moe import DeepSeekMoE

    torch.manual_seed(0)
    moe = DeepSeekMoE(cfg).to(BF16).cuda().train()
    d, E, k = cfg["emb_dim"], moe.num_routed, moe.top_k
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, T, d, generator=g).to(BF16).cuda().requires_grad_(True)
    dy = torch.randn(1, T, d, generator=g).to(BF16).cuda()
    h, dout = x.detach().view(T, d), dy.view(T, d)

    def whole():
        for p in moe.parameters():
            p.grad = None
        x.grad = None
        moe(x).backward(dy)

    # switch on (segmented GEMMs over all routed experts, no host read) and off (per-expert launches behind the read of the counts), same process, same
    # tensors; the shipped default last
    default, by_switch = ops_moe.SEGMENTED, {}
    for on in (not default, default):
        ops_moe.SEGMENTED = on
        whole()
        by_switch[on] = time_calls(whole, steps, warmup)
    arena = ops_dsmoe.ensure_arena(moe)
    idx, counts = moe._routed
    out = [dict(kind="layer", name="DeepSeekMoE forward + backward", tokens=T, counts=counts.tolist(), default_path="segmented" if default else "per-expert",
                segmented_ms_median=by_switch[True]["ms_median"], segmented_ms_min=by_switch[True]["ms_min"], segmented_ms_max=by_switch[True]["ms_max"],
                per_expert_ms_median=by_switch[False]["ms_median"], per_expert_ms_min=by_switch[False]["ms_min"], per_expert_ms_max=by_switch[False]["ms_max"],
                per_expert_over_segmented=by_switch[False]["ms_median"] / by_switch[True]["ms_median"], **by_switch[default])]
    wg8, bg8 = ops_moe.gate_operands(moe.gate, E)
    logits = K.gemm(L.GEMM_NT, h, wg8, bias=bg8)
    p, idx, w, s = KD.route_fwd(logits[:, :E], moe.biases, k)
    counts, offsets, slot, row_token, _ = KM.plan(idx, E)
    xs = KM.gather_rows(h, row_token)
    y = torch.randn(xs.shape, generator=g).to(BF16).cuda()
    dw = torch.randn(T, k, generator=g).cuda()
    scratch = moe.biases.clone()

    def router():
        a, b = ops_moe.gate_operands(moe.gate, E)
        lg = K.gemm(L.GEMM_NT, h, a, bias=b)
        KD.route_fwd(lg[:, :E], moe.biases, k)
        KD.bias_update(counts, scratch, moe.bias_update_rate)
        dl = torch.zeros((T, a.shape[0]), dtype=BF16, device="cuda")
        KM.route_bwd(dw, w, s, idx, p, dlogits=dl[:, :E])
        K.gemm(L.GEMM_NN, dl, a)
        K.gemm(L.GEMM_TN, dl, h, out_dtype=F32)
        K.colsum(dl)

    def plan():
        KM.plan(idx, E)

    def rows():
        KM.gather_rows(h, row_token)
        KM.combine_fwd(y, slot, w, h, shared=h)
        KM.combine_bwd(dout, row_token, slot, w, y)
        KM.combine_fwd(xs, slot)

    def shared():
        o, saved = ops_dsmoe.shared_forward(moe.shared_experts, h)
        wg = []
        ops_dsmoe.shared_backward(moe.shared_experts, arena, h, saved, dout, wg)
        ops_dsmoe._flush(wg)

    F_ = moe.routed_experts[0].hidden_dim

    def experts():  # the layer's own per-expert loops (ops_moe): the host read the layer pays, all forwards, then all backwards
        wg, routed = [], moe.routed_experts
        _, gus, acts, segs = ops_moe._experts_forward_loop(routed, "lin_gate", "lin1", arena, xs, counts.tolist(), F_)
        ops_moe._experts_backward_loop(routed, "lin_gate", "lin1", arena, xs, gus, acts, segs, y, F_, wg)
        ops_dsmoe._flush(wg)

    st = ops_moe.expert_stacks(moe, arena, moe.routed_experts, "lin_gate", "lin1")

    def experts_segmented():
        gu, a, _ = ops_moe.experts_forward(st, xs, counts, offsets, T * k, F_)
        ops_moe.experts_backward(st, arena, xs, gu, a, y, counts, offsets, T * k, F_)

    parts = [("router and bias update", router), ("plan", plan), ("rows", rows), ("routed expert GEMMs, per-expert launches (host read included)", experts),
             ("routed expert GEMMs, segmented (one launch per product, no host read)", experts_segmented)]
    if moe.num_shared > 0:
        parts.insert(3, ("shared experts", shared))
    for name, fn in parts:
        out.append(dict(kind="part", name=name, tokens=T, **time_calls(fn, steps, warmup)))
    return out


def measure_dense(cfg, T, steps, warmup):
    from llm_quest_amd.llama3_to_deepseekv3.deepseek_transformer_block import FFN

    torch.manual_seed(0)
    ffn = FFN(cfg).to(BF16).cuda().train()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, T, cfg["emb_dim"], generator=g).to(BF16).cuda().requires_grad_(True)
    dy = torch.randn(1, T, cfg["emb_dim"], generator=g).to(BF16).cuda()

    def step():
        for p in ffn.parameters():
            p.grad = None
        x.grad = None
        ffn(x).backward(dy)

    step()
    return dict(kind="dense", name=f"dense FFN (hidden {cfg['hidden_dim']}) forward + backward", tokens=T, **time_calls(step, steps, warmup))


def measure_step(cfg, label, batch, seq, steps, warmup):
    from llm_quest_amd.llama3_to_deepseekv3.deepseek_model import DeepSeekV3Model

    torch.manual_seed(0)
    torch.cuda.reset_peak_memory_stats()
    m = DeepSeekV3Model(cfg).to(BF16).cuda().train()
    with torch.no_grad():
        m.main_model.emb_layer.weight.normal_(0.0, 0.02)
    g = torch.Generator().manual_seed(1)
    tok = torch.randint(0, cfg["vocab_size"], (batch, seq + 3), generator=g).cuda()
    ids, tgt = tok[:, :seq].contiguous(), tok[:, 1 : seq + 1].contiguous()
    sx = [tok[:, 1 + k : seq + 1 + k].contiguous() for k in range(2)]
    sy = [tok[:, 2 + k : seq + 2 + k].contiguous() for k in range(2)]

    def step():
        for p in m.parameters():
            p.grad = None
        loss = m(ids, tgt, sx, sy)
        loss.backward()
        return loss.detach()

    from llm_quest_amd import ops_moe

    loss = float(step())
    default, by_switch = ops_moe.SEGMENTED, {}
    for on in (not default, default):  # (an all-dense model has no MoE layer: its two times show the run-to-run spread of this measurement)
        ops_moe.SEGMENTED = on
        step()
        by_switch[on] = time_calls(step, steps, warmup)
    r = dict(by_switch[default])
    r.update(segmented_ms_median=by_switch[True]["ms_median"], per_expert_ms_median=by_switch[False]["ms_median"],
             per_expert_over_segmented=by_switch[False]["ms_median"] / by_switch[True]["ms_median"])
    r.update(kind="step", model=label, batch=batch, seq=seq, tokens=batch * seq, loss=loss, parameters=sum(p.numel() for p in m.parameters()),
             peak_mem_gb=torch.cuda.max_memory_allocated() / 2**30)
    r["tokens_per_s"] = batch * seq / (r["ms_median"] * 1e-3)
    del m
    torch.cuda.empty_cache()
    return r


def main():
    from llm_quest_amd.config import DEEPSEEK_SMALL_CONFIG

    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--step-seq", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--model-steps", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deepseek_moe_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_deepseek_moe.py needs an MI355X: there is nothing to measure without one")
    results = []

    def emit(r):
        results.append(r)
        print(json.dumps(r), flush=True)

    cfg = dict(DEEPSEEK_SMALL_CONFIG)
    for r in measure_layer(cfg, args.tokens, args.steps, args.warmup):
        emit(r)
    emit(measure_dense(cfg, args.tokens, args.steps, args.warmup))
    if not args.skip_model:
        ctx = max(args.step_seq, cfg["context_length"])
        emit(measure_step(dict(cfg, mtp_depth=2, context_length=ctx), "DEEPSEEK_SMALL_CONFIG as written (3 dense + 9 DeepSeekMoE blocks, mtp_depth = 2)",
                          args.batch, args.step_seq, args.model_steps, 2))
        emit(measure_step(dict(cfg, num_ffn=cfg["n_layers"], mtp_depth=2, context_length=ctx), "dense DEEPSEEK_SMALL_CONFIG (num_ffn = n_layers = 12, mtp_depth = 2)",
                          args.batch, args.step_seq, args.model_steps, 2))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(note="tools/bench_deepseek_moe.py: one DeepSeekMoE layer forward + backward, its split, the dense FFN of the same config, and the training "
                                "step of DEEPSEEK_SMALL_CONFIG as written beside the all-dense one; device-event times, no profiler",
                           torch=torch.__version__, device=torch.cuda.get_device_name(0), results=results), f, indent=1)


if __name__ == "__main__":
    main()
