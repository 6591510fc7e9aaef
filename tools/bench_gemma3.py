"""Measure the Gemma3 path on the GPU.

    python tools/bench_gemma3.py [--batch 8] [--seq 4096] [--steps 5] [--warmup 2] [--out profiles/gemma3_bench.json]

(a) Attention kernels at the model's shape (bf16, 12 query heads over 6 kv heads, head_dim 64): the windowed kernels forward and
    forward + backward at W in {128, 512, 2048, S}, and beside them, on the same operands in the same process, the causal kernels that were
    there before: ``mi355_attn_generic_fwd/_bwd`` (the same structure without the band) and ``K.attn_fwd`` / ``K.attn_bwd`` (the tuned ones).
(b) The training step (forward + loss + backward) of Gemma3Model (emb 768, 12 layers, hidden 3072, vocab 50304) with window_size = 512,
    local_global_att_ratio = 5 against the same model with window_size = 0 (every layer on the tuned causal kernels).

Times are device events around whole calls, medians after warm-up, no profiler attached; one JSON line per measurement on stdout, all of
them in ``--out``.  The run ends with the condition the windowed kernels are held to: at W = 512 their forward + backward takes less time
than the generic causal kernels' (the same algorithm over about a quarter of the tiles).  Needs the GPU.
"""

import argparse
import gc
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16, F32 = torch.bfloat16, torch.float32
MODEL = dict(vocab_size=50304, emb_dim=768, n_heads=12, num_kv_groups=6, n_layers=12, hidden_dim=3072, rope_base=10000, dtype=BF16)


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


def measure_attention(B, S, Hq, Hkv, D, windows, reps):
    from llm_quest_amd import _lib as L
    from llm_quest_amd import kernels as K
    from llm_quest_amd import kernels_g3 as KG

    g = torch.Generator().manual_seed(3)
    rn = lambda h: torch.randn(B * S, h * D, generator=g).to(BF16).cuda()
    q, k, v, do = rn(Hq), rn(Hkv), rn(Hkv), rn(Hq)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    delta = torch.empty((B, Hq, S), dtype=F32, device="cuda")
    scale = D ** -0.5
    p = L.ptr

    def generic_fwd():
        o = torch.empty_like(q)
        lse = torch.empty((B, Hq, S), dtype=F32, device="cuda")
        L.require_gpu(q)
        L.call("mi355_attn_generic_fwd", B, S, Hq, Hkv, D, p(q), Hq * D, p(k), Hkv * D, p(v), Hkv * D, p(o), Hq * D, p(lse), None, scale)
        return o, lse

    def generic_bwd(o, lse):
        L.require_gpu(q)
        L.call("mi355_attn_generic_bwd", B, S, Hq, Hkv, D, p(q), Hq * D, p(k), Hkv * D, p(v), Hkv * D, p(o), Hq * D, p(do), Hq * D, p(lse), p(delta),
               p(dq), Hq * D, p(dk), Hkv * D, p(dv), Hkv * D, None, scale)

    variants = {"generic causal (mi355_attn_generic)": (generic_fwd, generic_bwd),
                "tuned causal (K.attn_fwd / K.attn_bwd)": (lambda: K.attn_fwd(q, k, v, B, S, Hq, Hkv, D), lambda o, lse: K.attn_bwd(q, k, v, o, do, lse, B, S, Hq, Hkv, D, dq, dk, dv))}
    for W in windows:
        variants[f"windowed W={W}"] = (lambda W=W: KG.swa_attn_fwd(q, k, v, B, S, Hq, Hkv, D, W),
                                       lambda o, lse, W=W: KG.swa_attn_bwd(q, k, v, o, do, lse, B, S, Hq, Hkv, D, W, dq, dk, dv))
    out = []
    for name, (fwd, bwd) in variants.items():
        o, lse = fwd()
        f = time_calls(fwd, reps, 3)
        fb = time_calls(lambda: bwd(*fwd()), reps, 3)
        out.append(dict(kind="attention", name=name, B=B, S=S, Hq=Hq, Hkv=Hkv, D=D, fwd_ms=f["ms_median"], fwd_ms_min=f["ms_min"], fwd_bwd_ms=fb["ms_median"],
                        fwd_bwd_ms_min=fb["ms_min"], reps=reps))
    return out


def measure_step(window, ratio, batch, seq, steps, warmup):
    from llm_quest_amd.llama3_to_gemma3.gemma3_model import Gemma3Model

    torch.manual_seed(0)
    cfg = dict(MODEL, context_length=seq, window_size=window, local_global_att_ratio=ratio)
    m = Gemma3Model(cfg).to(BF16).cuda().train()
    with torch.no_grad():
        m.emb_dict.weight.normal_(0.0, 0.02)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, cfg["vocab_size"], (batch, seq), generator=g).cuda()
    tgt = torch.randint(0, cfg["vocab_size"], (batch * seq,), generator=g).cuda()

    def step():
        for p in m.parameters():
            p.grad = None
        h = m.forward_hidden(ids)
        loss = m.lm_loss(h.reshape(-1, h.shape[-1]), tgt)
        loss.backward()
        return loss.detach()

    loss = float(step())
    r = time_calls(step, steps, warmup)
    r.update(kind="step", window_size=window, local_global_att_ratio=ratio, windowed_layers=sum(b.att.is_windowed for b in m.trf_blocks), batch=batch, seq=seq,
             tokens=batch * seq, loss=loss, peak_mem_gb=torch.cuda.max_memory_allocated() / 2**30)
    r["tokens_per_s"] = batch * seq / (r["ms_median"] * 1e-3)
    del m, step
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gemma3.py needs an MI355X: there is nothing to measure without one")
    results = []

    def emit(r):
        results.append(r)
        print(json.dumps(r), flush=True)

    windows = sorted({w for w in (128, 512, 2048, args.seq) if w <= args.seq})
    for r in measure_attention(args.batch, args.seq, MODEL["n_heads"], MODEL["num_kv_groups"], MODEL["emb_dim"] // MODEL["n_heads"], windows, args.kernel_reps):
        emit(r)
    by = {r["name"]: r for r in results}
    verdict = None
    if "windowed W=512" in by:
        w, gen = by["windowed W=512"]["fwd_bwd_ms"], by["generic causal (mi355_attn_generic)"]["fwd_bwd_ms"]
        verdict = dict(kind="condition", text="windowed forward + backward at W = 512 is faster than the generic causal kernels", windowed_ms=w, generic_ms=gen, holds=w < gen)
        emit(verdict)
    if not args.skip_model:
        emit(measure_step(512, 5, args.batch, args.seq, args.steps, args.warmup))
        emit(measure_step(0, 5, args.batch, args.seq, args.steps, args.warmup))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(note="tools/bench_gemma3.py: sliding-window attention kernels and the Gemma3Model training step; device-event times, no profiler",
                           torch=torch.__version__, device=torch.cuda.get_device_name(0), results=results), f, indent=1)
    if verdict is not None and not verdict["holds"]:
        raise SystemExit("the tile skipping is not working: windowed attention at W = 512 is not faster than the generic causal kernels")


if __name__ == "__main__":
    main()
