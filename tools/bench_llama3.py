"""Measure the Llama 3.2 path and the QK-Clip statistic on the GPU.

    python tools/bench_llama3.py [--batch 4] [--seq 1024] [--steps 10] [--warmup 3] [--out profiles/llama3_bench.json]

(a) ``mi355_attn_max_logit`` beside ``mi355_swa_attn_fwd`` with W >= S -- the plain kernel of the same 32-key tile layer doing both products and the
    softmax -- and, for context only, the tuned ``mi355_attn_fwd``, at (B, S, Hq, Hkv, D) = (4, 1024, 32, 8, 64) and (2, 4096, 24, 8, 128), same
    operands, same process, the variants alternating.
(b) The fused RoPE of the packed projection (one launch) beside two ``K.rope_apply`` calls plus the copies they need, at M = 4096, Hq = 32,
    Hkv = 8, D = 64.
(c) The training step (forward + loss + backward) of ``Llama3Model(LLAMA32_SMALL_CONFIG_1B)`` at ``context_length = --seq``, bf16, with
    ``track_max_attn_logit`` off and on, alternating: the difference is the price of the statistic per step.

Times are device events around whole calls, medians after warm-up, no profiler attached; one JSON line per measurement on stdout, all of them in
``--out`` together with the card's power cap and the power / shader clock sampled (amdgpu hwmon, read only) while the measurements ran.  The run ends
with the condition the max-logit kernel is held to: it does strictly less work than the plain attention forward in the same structure, so it must be
faster at both shapes.  Needs the GPU.
"""

import argparse
import glob
import json
import os
import sys
import threading
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16, F32 = torch.bfloat16, torch.float32
ATTN_SHAPES = [(4, 1024, 32, 8, 64), (2, 4096, 24, 8, 128)]


class Telemetry:
    """Power and shader clock of every visible amdgpu hwmon every 20 ms; ``result`` reports the card that drew the most."""

    def __init__(self):
        self.dirs = [os.path.dirname(p) for p in glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*/power1_input")]
        self.samples = {d: [] for d in self.dirs}
        self._stop = threading.Event()
        self._thread = threading.Thread(target=self._run, daemon=True)
        if self.dirs:
            self._thread.start()

    @staticmethod
    def _read(path):
        try:
            return int(open(path).read()) / 1e6
        except (OSError, ValueError):
            return None

    def _run(self):
        while not self._stop.is_set():
            for d in self.dirs:
                p, f = self._read(d + "/power1_input"), self._read(d + "/freq1_input")
                if p:
                    self.samples[d].append((p, f or 0.0))
            time.sleep(0.02)

    def result(self):
        self._stop.set()
        mean = {d: sum(x[0] for x in s) / len(s) for d, s in self.samples.items() if s}
        if not mean:
            return {"mean_W": None, "note": "no amdgpu hwmon telemetry is exposed here: clocks and power cap not recorded"}
        d = max(mean, key=mean.get)
        s = self.samples[d]
        return {"mean_W": round(mean[d], 1), "max_W": round(max(x[0] for x in s), 1), "cap_W": self._read(d + "/power1_cap"),
                "sclk_mean_MHz": round(sum(x[1] for x in s) / len(s)), "sclk_max_MHz": round(max(x[1] for x in s)), "samples": len(s),
                "source": "amdgpu hwmon power1_input / freq1_input every 20 ms over the whole run (idle gaps between measurements included)"}


def time_alternating(fns, reps, warmup):
    """{name: fn} timed round-robin (a, b, c, a, b, c, ...), each call between its own device events: medians and the spread."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in fns}
    for _ in range(reps):
        for n, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[n].append(a.elapsed_time(b))
    out = {}
    for n, ts in times.items():
        ts.sort()
        out[n] = {"ms_median": ts[len(ts) // 2], "ms_min": ts[0], "ms_max": ts[-1], "reps": reps}
    return out


def measure_attention(B, S, Hq, Hkv, D, reps):
    from llm_quest_amd import kernels as K
    from llm_quest_amd import kernels_g3 as KG
    from llm_quest_amd import kernels_llama as KL

    g = torch.Generator().manual_seed(3)
    rn = lambda h: torch.randn(B * S, h * D, generator=g).to(BF16).cuda()
    q, k, v = rn(Hq), rn(Hkv), rn(Hkv)
    # the two kernels that see the same logits agree on them: the row maxima of the plain forward's scores bound its lse from below
    m = KL.attn_max_logit(q, k, B, S, Hq, Hkv, D)
    _, lse = KG.swa_attn_fwd(q, k, v, B, S, Hq, Hkv, D, S)
    assert bool((m <= lse.amax(dim=(0, 2)) + 1e-3).all()) and bool(torch.isfinite(m).all())
    r = time_alternating({"max_logit": lambda: KL.attn_max_logit(q, k, B, S, Hq, Hkv, D),
                          "plain_fwd": lambda: KG.swa_attn_fwd(q, k, v, B, S, Hq, Hkv, D, S),
                          "tuned_fwd": lambda: K.attn_fwd(q, k, v, B, S, Hq, Hkv, D)}, reps, 5)
    flops_qk = 2.0 * B * Hq * D * S * (S + 1) / 2  # the causal half of q k^T
    return dict(kind="attention", B=B, S=S, Hq=Hq, Hkv=Hkv, D=D, max_logit_ms=r["max_logit"]["ms_median"], max_logit_ms_min=r["max_logit"]["ms_min"],
                max_logit_ms_max=r["max_logit"]["ms_max"], plain_fwd_ms=r["plain_fwd"]["ms_median"], plain_fwd_ms_min=r["plain_fwd"]["ms_min"],
                plain_fwd_ms_max=r["plain_fwd"]["ms_max"], tuned_fwd_ms=r["tuned_fwd"]["ms_median"], ratio_plain_over_max_logit=r["plain_fwd"]["ms_median"] / r["max_logit"]["ms_median"],
                max_logit_tflops_of_causal_qk=flops_qk / (r["max_logit"]["ms_median"] * 1e-3) / 1e12, reps=reps,
                note="max_logit includes its fold launch and the allocation of its partials; plain_fwd = mi355_swa_attn_fwd with W = S; tuned_fwd = mi355_attn_fwd, for context")


def measure_rope(M, Hq, Hkv, D, reps):
    from llm_quest_amd import kernels as K
    from llm_quest_amd import kernels_llama as KL

    g = torch.Generator().manual_seed(4)
    W = (Hq + 2 * Hkv) * D
    qkv = torch.randn(M, W, generator=g).to(BF16).cuda()
    ang = torch.rand(M, D, generator=g) * 6.28
    cos, sin = torch.cos(ang).cuda(), torch.sin(ang).cuda()
    pos = torch.randperm(M, generator=g).to(torch.int32).cuda()

    def separate():  # what the block would do without the fused kernel: rotate each head group through the (b, heads, s, head_dim) view, then pack it token-major
        q = K.rope_apply(qkv[:, : Hq * D].reshape(1, M, Hq, D).transpose(1, 2), cos, sin, pos)
        k = K.rope_apply(qkv[:, Hq * D : (Hq + Hkv) * D].reshape(1, M, Hkv, D).transpose(1, 2), cos, sin, pos)
        return q.transpose(1, 2).reshape(M, Hq * D).contiguous(), k.transpose(1, 2).reshape(M, Hkv * D).contiguous()

    q1, k1 = KL.rope_fwd(qkv, cos, sin, pos, Hq, Hkv, D)
    q2, k2 = separate()
    assert torch.equal(q1, q2) and torch.equal(k1, k2)
    r = time_alternating({"fused": lambda: KL.rope_fwd(qkv, cos, sin, pos, Hq, Hkv, D), "separate": separate}, reps, 5)
    moved = 2.0 * M * (Hq + Hkv) * D * 2  # bytes read + written by the fused kernel (bf16), tables aside
    return dict(kind="rope", M=M, Hq=Hq, Hkv=Hkv, D=D, fused_ms=r["fused"]["ms_median"], fused_ms_min=r["fused"]["ms_min"], separate_ms=r["separate"]["ms_median"],
                separate_ms_min=r["separate"]["ms_min"], ratio_separate_over_fused=r["separate"]["ms_median"] / r["fused"]["ms_median"],
                fused_gb_per_s=moved / (r["fused"]["ms_median"] * 1e-3) / 1e9, reps=reps)


def measure_step(batch, seq, steps, warmup):
    from llm_quest_amd.config import LLAMA32_SMALL_CONFIG_1B
    from llm_quest_amd.gpt_to_llama3.llama_model import Llama3Model

    torch.manual_seed(0)
    cfg = dict(LLAMA32_SMALL_CONFIG_1B, context_length=seq)
    with torch.device("cuda"):
        m = Llama3Model(cfg)
    m = m.to(BF16).train()
    with torch.no_grad():
        m.emb_dict.weight.normal_(0.0, 0.02)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, cfg["vocab_size"], (batch, seq), generator=g).cuda()
    tgt = torch.randint(0, cfg["vocab_size"], (batch * seq,), generator=g).cuda()

    def step(track):
        for blk in m.trf_blocks:
            blk.att.track_max_attn_logit = track
        for p in m.parameters():
            p.grad = None
        h = m.forward_hidden(ids)
        loss = m.lm_loss(h.reshape(-1, h.shape[-1]), tgt)
        loss.backward()
        return loss.detach()

    loss = float(step(False))
    r = time_alternating({"off": lambda: step(False), "on": lambda: step(True)}, steps, warmup)
    top = float(torch.stack([blk.att.max_attn_logit for blk in m.trf_blocks]).max())
    off, on = r["off"]["ms_median"], r["on"]["ms_median"]
    return dict(kind="step", model="LLAMA32_SMALL_CONFIG_1B", batch=batch, seq=seq, tokens=batch * seq, parameters=sum(p.numel() for p in m.parameters()), loss=loss,
                tracking_off_ms=off, tracking_off_ms_min=r["off"]["ms_min"], tracking_off_ms_max=r["off"]["ms_max"], tracking_on_ms=on, tracking_on_ms_min=r["on"]["ms_min"],
                tracking_on_ms_max=r["on"]["ms_max"], statistic_ms_per_step=on - off, statistic_share=(on - off) / off, tokens_per_s_off=batch * seq / (off * 1e-3),
                largest_tracked_logit=top, peak_mem_gb=torch.cuda.max_memory_allocated() / 2**30, steps=steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=30)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_llama3.py needs an MI355X: there is nothing to measure without one")
    tele = Telemetry()
    results = []

    def emit(r):
        results.append(r)
        print(json.dumps(r), flush=True)

    for shape in ATTN_SHAPES:
        emit(measure_attention(*shape, args.kernel_reps))
    slower = [r for r in results if r["kind"] == "attention" and not r["max_logit_ms"] < r["plain_fwd_ms"]]
    emit(dict(kind="condition", text="mi355_attn_max_logit is faster than mi355_swa_attn_fwd (W >= S) at both shapes", holds=not slower,
              ratios=[r["ratio_plain_over_max_logit"] for r in results if r["kind"] == "attention"]))
    emit(measure_rope(4096, 32, 8, 64, args.kernel_reps))
    if not args.skip_model:
        emit(measure_step(args.batch, args.seq, args.steps, args.warmup))
    power = tele.result()
    emit(dict(kind="telemetry", **power))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(note="tools/bench_llama3.py: the max-logit kernel beside the plain and the tuned attention forward, the fused RoPE, and the Llama 3.2 1B "
                                "training step with and without max-logit tracking; device-event times, no profiler",
                           torch=torch.__version__, device=torch.cuda.get_device_name(0), results=results), f, indent=1)
    if slower:
        raise SystemExit("mi355_attn_max_logit is not faster than the plain attention forward of the same tile layer: " + json.dumps(slower))


if __name__ == "__main__":
    main()
