"""Measure hyper-connection Qwen3 on the GPU: the training step (forward + loss + backward) of HyperQwen3Model at Qwen3-0.6B shapes,
against (a) the same model with the six fused kernels replaced by the reference's torch-op composition (``--unfused``; built from
tests/hyper_oracle.py, a measurement aid and not a product path) and (b) plain Qwen3Model; then each new kernel on its own against the
bytes it must move.

    python tools/bench_hyper.py [--batch 0] [--seq 1024] [--steps 5] [--warmup 2] [--out profiles/hyper_bench.json]

``--batch 0`` takes the largest of 32, 16, 8, 4 at which the UNFUSED step (the hungrier of the two) fits, so that every variant runs the
same shape.  Times are device events around whole steps (no profiler attached); one JSON line per measurement on stdout, all of them in
``--out``.  Needs the GPU: there is nothing to measure without one.
"""

import argparse
import gc
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

HBM_ACHIEVABLE = 6.3e12  # bytes / s, the rate DESIGN.md section 5 holds the row kernels against
N_STREAMS = 4


def config(seq):
    from llm_quest_amd.config import qwen3_config_creator

    cfg = qwen3_config_creator("0.6B")
    cfg["context_length"] = seq
    return cfg


def time_steps(fn, steps, warmup):
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


def unfused_forward_hidden(m, ids):
    """HyperQwen3Model.forward_hidden with every hyper-connection operation as the reference writes it: torch ops under autograd (a norm over
    all streams, fp32 casts, three small matmuls, three batched h @ x, the casts back, the add); the sub-layers stay on the HIP kernels."""
    import hyper_oracle as HO
    from llm_quest_amd import ops

    m._build_arenas()
    x = m.emb_dict(ids)
    B, S, _ = x.shape
    cos, sin = m._rope_tables()
    n = m.expansion_rate
    x = x.unsqueeze(-2).expand(-1, -1, n, -1)
    for blk in m.trf_blocks:
        blk._build_arenas()
        for hc, norm, sub in ((blk.hc_attn, blk.norm1, lambda h: blk.att(h, m.mask, cos, sin)), (blk.hc_ffn, blk.norm2, blk.ffn)):
            c = HO.Coeffs(hc["norm"].weight, hc["res"].linear.weight, hc["pre"].linear.weight, hc["post"].linear.weight, hc["res"].factor,
                          hc["pre"].factor, hc["post"].factor, hc["res"].bias, hc["pre"].bias, hc["post"].bias)
            R, P, H, _ = HO.width_fwd(x, c)
            x = HO.depth_fwd(sub(norm(P)), H[..., n + 1, :], R)
    return m.final_norm(x.sum(dim=-2))


def step_fn(m, ids, tgt, forward_hidden=None):
    def step():
        for p in m.parameters():
            p.grad = None
        h = forward_hidden(m, ids) if forward_hidden is not None else m.forward_hidden(ids)
        loss = m.lm_loss(h.reshape(-1, h.shape[-1]), tgt)
        loss.backward()
        return loss.detach()

    return step


def build(kind, cfg):
    from llm_quest_amd.common.hyper_connections.hyper_qwen3 import HyperQwen3Model
    from llm_quest_amd.qwen.qwen3.qwen3_model import Qwen3Model

    torch.manual_seed(0)
    m = Qwen3Model(dict(cfg)) if kind == "plain" else HyperQwen3Model(dict(cfg), "hc", N_STREAMS)
    if kind != "plain":  # off the initial values, as in the test fixture: at initialisation tanh(0) makes half the arithmetic trivial
        import hyper_oracle as HO

        HO.perturb_coefficients(list(m.named_parameters()), torch.Generator().manual_seed(0))
    return m.cuda().train()


def free():
    gc.collect()
    torch.cuda.empty_cache()


def measure_step(kind, cfg, batch, seq, steps, warmup):
    m = build(kind, cfg)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, cfg["vocab_size"], (batch, seq), generator=g).cuda()
    tgt = torch.randint(0, cfg["vocab_size"], (batch * seq,), generator=g).cuda()
    fn = step_fn(m, ids, tgt, unfused_forward_hidden if kind == "unfused" else None)
    loss = float(fn())
    r = time_steps(fn, steps, warmup)
    r.update(kind=kind, batch=batch, seq=seq, tokens=batch * seq, loss=loss, peak_mem_gb=torch.cuda.max_memory_allocated() / 2**30)
    r["tokens_per_s"] = batch * seq / (r["ms_median"] * 1e-3)
    del m, fn
    free()
    torch.cuda.reset_peak_memory_stats()
    return r


def measure_kernels(T, n, d, reps):
    """Each new kernel alone at the step's shape.  'bytes' is what the kernel must move once (bf16 streams in and out; the fp32 coefficients,
    weights and partial rows are below 1 % of it); gbps = bytes / time, share = gbps over the achievable HBM rate."""
    import hyper_oracle as HO
    from llm_quest_amd import kernels_hc as KH

    X, c, Y, dOut, dP, dh_post = HO.make_operands(T, n, d, seed=2)
    c = KH.Coeffs(*[None if t is None else t.cuda() for t in c])
    X, Y, dOut, dP, dh_post = X.cuda(), Y.cuda(), dOut.cuda(), dP.cuda(), dh_post.cuda()
    R, P, H, TH, rstd = KH.width_fwd(X, c)
    row = T * d * 2  # bytes of one [T, d] bf16 tensor
    cases = {
        "hc_width_fwd": (lambda: KH.width_fwd(X, c), row * (2 * n + 1)),
        "hc_depth_fwd": (lambda: KH.depth_fwd(Y, H, R), row * (2 * n + 1)),
        "hc_depth_bwd": (lambda: KH.depth_bwd(dOut, Y, H), row * (n + 2)),
        "hc_width_bwd (+ fold of the partials)": (lambda: KH.width_bwd(dOut, dP, dh_post, X, H, TH, rstd, c), row * (3 * n + 1)),
        "hc_stream_sum": (lambda: KH.stream_sum(X), row * (n + 1)),
        "hc_stream_broadcast": (lambda: KH.stream_broadcast(Y, n), row * (n + 1)),
    }
    out = []
    for name, (fn, nbytes) in cases.items():
        r = time_steps(fn, reps, 3)
        gbps = nbytes / (r["ms_median"] * 1e-3) / 1e9
        out.append(dict(kind="kernel", name=name, T=T, n=n, d=d, bytes=nbytes, ms_median=r["ms_median"], ms_min=r["ms_min"], gbps=gbps,
                        share_of_achievable_hbm=gbps * 1e9 / HBM_ACHIEVABLE))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--unfused", action="store_true", help="measure ONLY the torch-op composition of the hyper-connections (default: all variants)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hyper.py needs an MI355X: there is nothing to measure without one")
    cfg = config(args.seq)
    results = []

    def emit(r):
        results.append(r)
        print(json.dumps(r), flush=True)

    batch, first = args.batch, None
    if batch == 0:
        for cand in (32, 16, 8, 4):
            try:
                first = measure_step("unfused", cfg, cand, args.seq, args.steps, args.warmup)
                batch = cand
                break
            except torch.cuda.OutOfMemoryError:
                emit(dict(kind="unfused", batch=cand, seq=args.seq, oom=True))
                free()
        if first is None:
            raise SystemExit("the unfused step does not fit at batch 4")
    emit(first if first is not None else measure_step("unfused", cfg, batch, args.seq, args.steps, args.warmup))
    if not args.unfused:
        emit(measure_step("fused", cfg, batch, args.seq, args.steps, args.warmup))
        emit(measure_step("plain", cfg, batch, args.seq, args.steps, args.warmup))
        for r in measure_kernels(batch * args.seq, N_STREAMS, cfg["emb_dim"], args.kernel_reps):
            emit(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(note="tools/bench_hyper.py: HyperQwen3Model (hc, n = 4) at Qwen3-0.6B shapes; device-event times, no profiler",
                           torch=torch.__version__, device=torch.cuda.get_device_name(0), results=results), f, indent=1)


if __name__ == "__main__":
    main()
