"""Measure the DeepSeek-V3 (Multi-head Latent Attention) path on the GPU.

    python tools/bench_deepseek.py [--steps 5] [--warmup 2] [--kernel-reps 10] [--out profiles/deepseek_bench.json]

MLA forward + backward, RoPE included on every side, at B = 8, S in {1024, 4096}, Hq = 12 at (Dn, Dr) = (64, 32) and Hq = 16 at (128, 64),
on the same operands in the same process:
(a) the MLA kernels: ``mla_rope_fwd`` -> ``mla_attn_fwd`` -> ``mla_attn_bwd`` -> ``mla_rope_bwd`` (head sum of dk_rope inside);
(b) the composition that was available before them: ``K.rope_apply`` on the two rotary parts, concatenate [q_nope | q_rope] and
    [k_nope | k_rope expanded to the heads], zero-pad Q, K and V to 128 (256 for Dn = 128), ``mi355_attn_dropout_fwd/_bwd`` plain causal with
    p = 0, slice the results, sum dk_rope over heads, rotate back -- every copy included;
(c) for (64, 32) only, the same padding on the tuned ``mi355_attn_fwd/_bwd`` at head dim 128.
Then the training step (forward + loss + backward) of the dense ``DEEPSEEK_SMALL_CONFIG`` (num_ffn = n_layers, mtp_depth = 2).

Times are device events around whole calls, medians after warm-up, no profiler attached; one JSON line per measurement on stdout, all of
them in ``--out``.  The run ends with the condition the MLA kernels are held to: (a) is faster than (b) at every shape (the same structure
doing strictly less work).  (c) is reported, not gated: the tuned kernels are pipelined, the MLA kernels are not.  Needs the GPU.
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


def measure_attention(B, S, H, Dn, Dr, reps):
    from llm_quest_amd import kernels as K
    from llm_quest_amd import kernels_mla as KM
    from llm_quest_amd.common.rope import RoPE

    T, DK, P = B * S, Dn + Dr, 128 if Dn == 64 else 256
    scale = DK ** -0.5
    g = torch.Generator().manual_seed(3)
    rn = lambda w: torch.randn(T, w, generator=g).to(BF16).cuda()
    q_nope, q_rope_pre, k_nope, k_rope_pre, v, do = rn(H * Dn), rn(H * Dr), rn(H * Dn), rn(Dr), rn(H * Dn), rn(H * Dn)
    cos, sin = [t.cuda() for t in RoPE.compute_angles(base=10000, head_dim=Dr, ctx_len=S)]

    def mla():
        qr, kr = KM.mla_rope_fwd(q_rope_pre, k_rope_pre, S, H, Dr, cos, sin)
        o, lse = KM.mla_attn_fwd(q_nope, qr, k_nope, kr, v, B, S, H, Dn, Dr)
        dqn, dqr, dkn, dkh, dv = KM.mla_attn_bwd(q_nope, qr, k_nope, kr, v, o, do, lse, B, S, H, Dn, Dr)
        gq, gk = KM.mla_rope_bwd(dqr, dkh, S, H, Dr, cos, sin)
        return o, dqn, gq, dkn, gk, dv

    heads4 = lambda t, h: t.view(B, S, h, Dr).transpose(1, 2)  # (b, heads, s, Dr) view of a token-major tensor

    def padded(fwd, bwd):
        def run():
            qr = K.rope_apply(heads4(q_rope_pre, H), cos, sin).transpose(1, 2).reshape(T, H, Dr)
            kr = K.rope_apply(heads4(k_rope_pre, 1), cos, sin).transpose(1, 2).reshape(T, 1, Dr)
            Q, Kp, V, dO = [torch.zeros(T, H, P, dtype=BF16, device="cuda") for _ in range(4)]
            Q[:, :, :Dn], Q[:, :, Dn:DK] = q_nope.view(T, H, Dn), qr
            Kp[:, :, :Dn], Kp[:, :, Dn:DK] = k_nope.view(T, H, Dn), kr  # the shared key copied to every head
            V[:, :, :Dn], dO[:, :, :Dn] = v.view(T, H, Dn), do.view(T, H, Dn)
            Q, Kp, V, dO = [t.view(T, H * P) for t in (Q, Kp, V, dO)]
            o, lse = fwd(Q, Kp, V)
            dQ, dK, dV = torch.empty_like(Q), torch.empty_like(Kp), torch.empty_like(V)
            bwd(Q, Kp, V, o, dO, lse, dQ, dK, dV)
            dQ, dK, dV = dQ.view(T, H, P), dK.view(T, H, P), dV.view(T, H, P)
            ctx = o.view(T, H, P)[:, :, :Dn].reshape(T, H * Dn)
            dqn, dkn, dv = [t[:, :, :Dn].reshape(T, H * Dn) for t in (dQ, dK, dV)]
            dqr = dQ[:, :, Dn:DK].reshape(T, H * Dr)
            dkr = dK[:, :, Dn:DK].float().sum(dim=1).to(BF16)
            gq = K.rope_apply(heads4(dqr, H), cos, sin, transpose=True)
            gk = K.rope_apply(heads4(dkr, 1), cos, sin, transpose=True)
            return ctx, dqn, gq.transpose(1, 2).reshape(T, H * Dr), dkn, gk.transpose(1, 2).reshape(T, Dr), dv

        return run

    variants = {"a: MLA kernels": mla,
                f"b: concat + pad to {P} + generic plain causal (mi355_attn_dropout, p = 0)": padded(
                    lambda Q, Kp, V: K.attn_dropout_fwd(Q, Kp, V, B, S, H, H, P, 0.0, 0, 0, causal=True, scale=scale),
                    lambda Q, Kp, V, o, dO, lse, dQ, dK, dV: K.attn_dropout_bwd(Q, Kp, V, o, dO, lse, B, S, H, H, P, dQ, dK, dV, 0.0, 0, 0, causal=True, scale=scale))}
    if Dn == 64:
        variants["c: concat + pad to 128 + tuned causal (mi355_attn)"] = padded(
            lambda Q, Kp, V: K.attn_fwd(Q, Kp, V, B, S, H, H, P, scale=scale),
            lambda Q, Kp, V, o, dO, lse, dQ, dK, dV: K.attn_bwd(Q, Kp, V, o, dO, lse, B, S, H, H, P, dQ, dK, dV, scale=scale))
    out, first = [], None
    for name, fn in variants.items():
        res = fn()
        if first is None:
            first = res
        else:  # the three sides compute the same function: a gross disagreement means a side is not measuring what it says
            for x, y in zip(first, res):
                d = float((x.float() - y.float()).norm() / y.float().norm().clamp_min(1e-30))
                if not d < 3e-2:
                    raise SystemExit(f"{name}: disagrees with the MLA kernels by {d:.3e}")
        r = time_calls(fn, reps, 3)
        out.append(dict(kind="attention", name=name, variant=name[0], B=B, S=S, Hq=H, Dn=Dn, Dr=Dr, fwd_bwd_ms=r["ms_median"], fwd_bwd_ms_min=r["ms_min"],
                        fwd_bwd_ms_max=r["ms_max"], reps=reps))
        del res
    del first
    gc.collect()
    torch.cuda.empty_cache()
    return out


def measure_step(batch, seq, steps, warmup):
    from llm_quest_amd.config import DEEPSEEK_SMALL_CONFIG
    from llm_quest_amd.llama3_to_deepseekv3.deepseek_model import DeepSeekV3Model

    torch.manual_seed(0)
    cfg = dict(DEEPSEEK_SMALL_CONFIG, num_ffn=DEEPSEEK_SMALL_CONFIG["n_layers"], mtp_depth=2, context_length=max(seq, DEEPSEEK_SMALL_CONFIG["context_length"]))
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

    loss = float(step())
    r = time_calls(step, steps, warmup)
    r.update(kind="step", model="dense DEEPSEEK_SMALL_CONFIG (num_ffn = n_layers = 12, mtp_depth = 2)", batch=batch, seq=seq, tokens=batch * seq, loss=loss,
             parameters=sum(p.numel() for p in m.parameters()), peak_mem_gb=torch.cuda.max_memory_allocated() / 2**30)
    r["tokens_per_s"] = batch * seq / (r["ms_median"] * 1e-3)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seqs", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--step-seq", type=int, default=512)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deepseek_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_deepseek.py needs an MI355X: there is nothing to measure without one")
    results = []

    def emit(r):
        results.append(r)
        print(json.dumps(r), flush=True)

    holds = True
    for S in args.seqs:
        for H, Dn, Dr in ((12, 64, 32), (16, 128, 64)):
            rs = measure_attention(args.batch, S, H, Dn, Dr, args.kernel_reps)
            for r in rs:
                emit(r)
            by = {r["variant"]: r["fwd_bwd_ms"] for r in rs}
            ok = by["a"] < by["b"]
            holds = holds and ok
            emit(dict(kind="condition", text="MLA kernels forward + backward faster than the padded generic composition", B=args.batch, S=S, Hq=H, Dn=Dn, Dr=Dr,
                      a_ms=by["a"], b_ms=by["b"], c_ms=by.get("c"), holds=ok))
    if not args.skip_model:
        emit(measure_step(args.batch, args.step_seq, args.steps, args.warmup))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(note="tools/bench_deepseek.py: MLA forward + backward (RoPE included) against the padded compositions, and the dense DeepSeek-V3 "
                                "training step; device-event times, no profiler", torch=torch.__version__, device=torch.cuda.get_device_name(0), results=results),
                      f, indent=1)
    if not holds:
        raise SystemExit("the MLA kernels are not faster than the padded generic composition at every shape: find the defect, do not ship it")


if __name__ == "__main__":
    main()
