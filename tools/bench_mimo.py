"""Measure the MiMo-V2-Flash path on the GPU.

    python tools/bench_mimo.py [--batch 8] [--steps 8] [--warmup 3] [--out profiles/mimo_bench.json]

(a) Sink attention forward and forward + backward (bf16) at MIMO_V2_SMALL_CONFIG's sliding-window shape (S = 512, 12 query heads over 4 kv heads,
    head dims 64 / 32, W = 128, a sink) and at a long shape (S = 4096), each beside the same kernels at W = S.  (``kernels_g3.swa_attn_*`` are
    the same kernels at DV = D without a sink -- csrc/attention_band.hip -- so there is no windowed counterpart to time them against.)
(b) The training step (forward + loss + backward, MTP on) of ``MiMoModel(MIMO_V2_SMALL_CONFIG).to(bfloat16)`` as written, against the same
    model with window_size = context_length (every layer walks the whole causal triangle).

Times are device events around windows of several calls, medians after warm-up, the variants of one comparison alternating inside one process, no
profiler attached; one JSON line per measurement on stdout, all of them in ``--out``.  Needs the GPU: without one there is nothing to measure.
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


def time_alternating(fns, rounds, warmup, inner):
    """{name: fn} -> {name: stats}: every round times each variant once (``inner`` calls between two events), so drift hits all alike."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            times[n].append(a.elapsed_time(b) / inner)
    out = {}
    for n, ts in times.items():
        ts.sort()
        out[n] = {"ms_median": ts[len(ts) // 2], "ms_min": ts[0], "ms_max": ts[-1], "rounds": rounds, "calls_per_round": inner}
    return out


def attention_flops(B, S, Hq, D, DV, W, backward):
    """Matrix operations over the visible (query, key) pairs only: QK^T and PV forward; S, dP, dV, dK, dQ products backward (S and dP run in both passes)."""
    w = min(W, S)
    pairs = B * Hq * (w * (w + 1) // 2 + (S - w) * w)
    fwd = 2 * pairs * (D + DV)
    bwd = 2 * pairs * (2 * D + DV) + 2 * pairs * (2 * D + 2 * DV)  # the dQ pass (S, dP, dQ), then the dK/dV pass (S, dP, dV, dK)
    return fwd + (bwd if backward else 0)


def measure_attention(B, S, Hq, Hkv, D, DV, W, sink, rounds, inner):
    from llm_quest_amd import kernels_mimo as KM

    g = torch.Generator().manual_seed(3)
    rn = lambda width: torch.randn(B * S, width, generator=g).to(BF16).cuda()
    q, k, v, do = rn(Hq * D), rn(Hkv * D), rn(Hkv * DV), rn(Hq * DV)
    z = torch.randn(Hq, generator=g).cuda() if sink else None
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)

    def mimo(W):
        fwd = lambda: KM.sink_attn_fwd(q, k, v, B, S, Hq, Hkv, D, DV, W, sink=z)
        return fwd, lambda: KM.sink_attn_bwd(q, k, v, *_ol(fwd()), B, S, Hq, Hkv, D, DV, W, sink=z, dq=dq, dk=dk, dv=dv)

    def _ol(r):
        return r[0], do, r[1]

    variants = {f"sink attention W={W}": mimo(W), f"sink attention W=S={S}": mimo(S)}
    f = time_alternating({n: fb[0] for n, fb in variants.items()}, rounds, 3, inner)
    fb = time_alternating({n: fb[1] for n, fb in variants.items()}, rounds, 3, inner)
    out = []
    for n in variants:
        w = S if "W=S" in n or n.endswith(f"W={S}") else W
        r = dict(kind="attention", name=n, B=B, S=S, Hq=Hq, Hkv=Hkv, D=D, DV=DV, sink=bool(sink), fwd_ms=f[n]["ms_median"], fwd_ms_min=f[n]["ms_min"],
                 fwd_bwd_ms=fb[n]["ms_median"], fwd_bwd_ms_min=fb[n]["ms_min"], rounds=rounds, calls_per_round=inner)
        r["fwd_tflops"] = attention_flops(B, S, Hq, D, DV, w, False) / (r["fwd_ms"] * 1e-3) / 1e12
        r["fwd_bwd_tflops"] = attention_flops(B, S, Hq, D, DV, w, True) / (r["fwd_bwd_ms"] * 1e-3) / 1e12
        out.append(r)
    return out


def build_step(window, batch):
    from llm_quest_amd.config import MIMO_V2_SMALL_CONFIG
    from llm_quest_amd.xiaomi.mimo_v2_flash_model import MiMoModel

    torch.manual_seed(0)
    cfg = dict(MIMO_V2_SMALL_CONFIG)
    if window is not None:
        cfg["window_size"] = window
    m = MiMoModel(cfg).to(BF16).cuda().train()
    with torch.no_grad():
        m.main_model.emb_layer.weight.normal_(0.0, 0.02)
    g = torch.Generator().manual_seed(1)
    seq = cfg["context_length"]
    ids = torch.randint(0, cfg["vocab_size"], (batch, seq), generator=g).cuda()
    tgt = torch.randint(0, cfg["vocab_size"], (batch, seq), generator=g).cuda()

    def step():
        for p in m.parameters():
            p.grad = None
        loss = m(ids, tgt)
        loss.backward()
        return loss.detach()

    return m, cfg, step


def measure_steps(batch, steps, warmup):
    from llm_quest_amd.config import MIMO_V2_SMALL_CONFIG

    ctx = MIMO_V2_SMALL_CONFIG["context_length"]
    built = {"as written": build_step(None, batch), f"window_size = context_length = {ctx}": build_step(ctx, batch)}
    losses = {n: float(b[2]()) for n, b in built.items()}
    t = time_alternating({n: b[2] for n, b in built.items()}, steps, warmup, 1)
    out = []
    for n, (m, cfg, _) in built.items():
        r = dict(t[n], kind="step", name=n, window_size=cfg["window_size"], windowed_layers=sum(b.use_sliding_window for b in m.main_model.layers) + len(m.mtp_modules),
                 batch=batch, seq=ctx, tokens=batch * ctx, loss=losses[n], mtp_depth=cfg["mtp_depth"], peak_mem_gb_both_models=torch.cuda.max_memory_allocated() / 2**30)
        r["tokens_per_s"] = batch * ctx / (r["ms_median"] * 1e-3)
        out.append(r)
    del built
    gc.collect()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-rounds", type=int, default=9)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mimo.py needs an MI355X: there is nothing to measure without one")
    from llm_quest_amd.config import MIMO_V2_SMALL_CONFIG as C

    results = []

    def emit(r):
        results.append(r)
        print(json.dumps(r), flush=True)

    Hq, Hkv, D, DV, W = C["n_heads"], C["num_swa_kv_groups"], C["head_dim"], C["value_head_dim"], C["window_size"]
    shapes = [(args.batch, C["context_length"], 40), (2, 4096, 8)]  # (B, S, calls per timed window)
    for B, S, inner in shapes:
        for r in measure_attention(B, S, Hq, Hkv, D, DV, W, True, args.kernel_rounds, inner):
            emit(r)
    if not args.skip_model:
        for r in measure_steps(args.batch, args.steps, args.warmup):
            emit(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(note="tools/bench_mimo.py: sink attention kernels and the MiMoModel(MIMO_V2_SMALL_CONFIG) training step; device-event times, "
                                "variants alternating in one process, no profiler",
                           torch=torch.__version__, device=torch.cuda.get_device_name(0), results=results), f, indent=1)


if __name__ == "__main__":
    main()
