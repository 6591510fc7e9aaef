"""Time the Reinforced Attention Learning kernels on the GPU.

    python tools/bench_ral.py [--batch 2] [--seq 1024] [--heads 32] [--kv 8] [--dim 64] [--reps 10] [--warmup 3]

One JSON line per measurement on stdout: the prepared distribution from q, k (``mi355_ral_qk_prepare_fwd``) and its backward, the same distribution
from materialised weights (``mi355_ral_prepare_fwd``; the softmax that produces the weights is not part of the time), the JSD rows, the reduction and
the whole loss, forward + backward, through the public interface on both entries.  Times are device events around whole calls, medians after
warm-up, no profiler attached.  Prints times and asserts none.  Needs the GPU.
"""

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16, F32 = torch.bfloat16, torch.float32


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv", type=int, default=8)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from llm_quest_amd import kernels_ral as KR
    from llm_quest_amd.common import reinforced_attention_learning as R

    B, S, Hq, Hkv, D = a.batch, a.seq, a.heads, a.kv, a.dim
    g = torch.Generator().manual_seed(0)
    rows = lambda h: torch.randn(B * S, h * D, generator=g).to(BF16).cuda()
    q, k, qo, ko = rows(Hq), rows(Hkv), rows(Hq), rows(Hkv)
    adv = torch.randn(B, generator=g).cuda()
    lm = torch.ones(B, S, device="cuda")
    P, Z, lse = KR.qk_prepare_fwd(q, k, B, S, Hq, Hkv, D)
    Q = KR.qk_prepare_fwd(qo, ko, B, S, Hq, Hkv, D)[0]
    jsd = KR.jsd_fwd(P, Q)
    _, w = KR.reduce(jsd, adv, lm)
    dP = KR.jsd_bwd(P, Q, w)
    da = KR.renorm_bwd(P, Z, dP, True)
    s = (q.view(B, S, Hq, D).transpose(1, 2).float() @ k.view(B, S, Hkv, D).transpose(1, 2).float().repeat_interleave(Hq // Hkv, dim=1).mT) * D ** -0.5
    wts = torch.softmax(s.masked_fill(torch.ones(S, S, dtype=torch.bool, device="cuda").triu_(1), float("-inf")), dim=-1)
    del s

    def whole(policy):
        def run():
            leaves = [t.detach().requires_grad_(True) for t in policy]
            Pp = R.prepare_attention_weights_from_qk(*leaves, B, S, Hq, Hkv, D) if len(leaves) == 2 else leaves[0]
            R.attention_divergence_loss(Pp, Q, adv, lm).backward()

        return run

    cases = {
        "qk_prepare_fwd": lambda: KR.qk_prepare_fwd(q, k, B, S, Hq, Hkv, D),
        "qk_prepare_bwd": lambda: KR.qk_prepare_bwd(q, k, da, lse, B, S, Hq, Hkv, D),
        "prepare_fwd (weights)": lambda: KR.prepare_fwd(wts),
        "prepare_bwd (weights)": lambda: KR.prepare_bwd(da, Hq, F32),
        "renorm_bwd": lambda: KR.renorm_bwd(P, Z, dP, True),
        "jsd_fwd": lambda: KR.jsd_fwd(P, Q),
        "jsd_bwd": lambda: KR.jsd_bwd(P, Q, w),
        "reduce": lambda: KR.reduce(jsd, adv, lm),
        "loss fwd+bwd from q, k": whole((q, k)),
        "loss fwd+bwd from weights": whole((wts,)),
    }
    for name, fn in cases.items():
        med, lo, hi = median_ms(fn, a.reps, a.warmup)
        print(json.dumps({"what": name, "B": B, "S": S, "Hq": Hq, "Hkv": Hkv, "D": D, "ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4)}))


if __name__ == "__main__":
    main()
