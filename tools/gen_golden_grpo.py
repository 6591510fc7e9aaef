"""Generate the GRPO fixture by running the REFERENCE on the CPU.  Run from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_grpo.py --ref <path to the reference checkout> [--out tests/golden]

The reference package is imported at run time from ``--ref`` (nothing of it is copied here, and it is never present where the GPU tests run).
Output, tensors and names only:

  * ``grpo_tiny.safetensors`` (under 1 MiB).  Case ``A``: B = 6 in two groups of 3, S = 9, V = 40; case ``B``: B = 2, S = 4, V = 1000, one group of 2.
    Inputs (``<case>.in.*``): bf16 logits 3 N(0, 1), ids, the loss mask (different start and end per sequence; in A sequence 4 is masked out entirely),
    ``mask_gspo`` (the same with two live tokens in sequence 4: an empty mask is NaN there), old / reference log-probs = the fp64 policy log-probs +
    0.3 N(0, 1), advantages.  For all five variants, with and without ``unbiased_kl_estimate`` and with and without the off-policy mask
    (``<case>.<variant>.u<0|1>.m<0|1>.*``), composed as the training loop composes the reference's functions (:1082-1111, the mask from
    ``off_policy_seq_mask`` on the loop's own ``kl_div``): ``loss32`` and ``dlogits32`` (rows 0 .. S - 2) of its fp32 run, ``loss16`` (and for case A
    ``dlogits16``) of its bf16 run, and the fp32 run's ``policy_ratio``, ``kl_div`` and ``opm``.  For gspo the loop's KL is the plain k3 whatever
    the flag (a (B,) ratio cannot weigh a (B, T) KL).
  * ``z.*``: rewards, and ``z_scores`` with / without ``dr_grpo`` and the phantom reward; ``bt.*``: ``bt_loss`` operands and values.
  * ``grpo_signatures.json``: parameter names and defaults of every public name, the seeds, ``delta`` per case, the measured floors (distance of the
    reference's bf16 run to its fp32 run).

Conditions (not measurements) the inputs must meet; per case the seed is the first of 0, 1, 2, ... that meets them, and it is stored:
  * no fp64 ratio (per token, and per sequence under ``mask_gspo``) lies within 1e-3 of ``1 - min_clip`` or ``1 + max_clip``;
  * no advantage is 0;
  * the off-policy mask holds a True and a False in every configuration: ``delta`` is chosen midway between two of the fixture's own per-sequence
    mean KLs and stored, and no mean KL of any configuration lies within 1e-3 of it.
"""

import argparse
import inspect
import json
import os
import sys

os.environ.setdefault("HF_HUB_OFFLINE", "1")

import torch
from safetensors.torch import save_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import grpo_oracle as GO  # noqa: E402

CASES = {"A": dict(B=6, S=9, V=40, num_samples=3, dead_seq=4), "B": dict(B=2, S=4, V=1000, num_samples=2, dead_seq=None)}
MAX_GEN = {"A": 8, "B": 3}
PUBLIC = ("bt_loss", "z_scores", "log_probs_per_token", "log_probs_per_token_optimized", "log_probs_per_seq", "kl_div_per_token", "off_policy_seq_mask")
METHODS = ("compute", "_compute_clipped_surrogate", "_compute_sapo_surrogate", "_compute_gspo_loss", "_aggregate")


def sig(fn):
    return [[n, None if p.default is inspect.Parameter.empty else repr(p.default)] for n, p in inspect.signature(fn).parameters.items()]


def gspo_mask(mask, dead_seq):
    m = mask.clone()
    if dead_seq is not None:
        m[dead_seq, 2:4] = True
    return m


def ref_run(RG, inp, mask, num_samples, max_gen, variant, unbiased, delta, dtype):
    """The loop's composition (:1082-1111) in ``dtype``, then backward to the logits."""
    logits = inp["logits"].to(dtype).detach().clone().requires_grad_(True)
    old, ref, adv = inp["old"].to(dtype), inp["ref"].to(dtype), inp["adv"].to(dtype)
    pol = RG.log_probs_per_token(logits=logits, inputs=inp["ids"])
    if variant == "gspo":
        ratio = torch.exp(RG.log_probs_per_seq(pol, mask) - RG.log_probs_per_seq(old, mask))
    else:
        ratio = torch.exp(pol - old)
    if unbiased and variant != "gspo":
        kl = RG.kl_div_per_token(pol, ref, policy_ratio=ratio)
    else:
        kl = RG.kl_div_per_token(pol, ref)
    opm = None if delta is None else RG.off_policy_seq_mask(kl.detach(), adv, mask, delta=delta)
    loss = RG.GRPOLoss.compute(policy_ratio=ratio, advantages=adv, loss_mask=mask, min_clip=GO.MIN_CLIP, max_clip=GO.MAX_CLIP, beta=GO.BETA, kl_div=kl,
                               num_samples=num_samples, max_gen=max_gen, variant=variant, off_policy_mask=opm)
    loss.backward()
    m = mask.to(dtype)
    mean_kl = (kl.detach() * m).sum(-1) / m.sum(-1).clamp(min=1)
    return {"loss": loss.detach(), "dlogits": logits.grad[:, :-1].contiguous(), "ratio": ratio.detach(), "kl": kl.detach(),
            "opm": torch.ones(mask.shape[0], dtype=torch.bool) if opm is None else opm.view(-1), "mean_kl": mean_kl}


def build_case(RG, name, spec, seed):
    inp = GO.fixture_inputs(spec["B"], spec["S"], spec["V"], spec["num_samples"], seed, dead_seq=spec["dead_seq"])
    mg = gspo_mask(inp["mask"], spec["dead_seq"])
    delta = GO.midway_delta(inp, inp["mask"])
    if delta is None:
        return None, ["no delta separates two sequences"]
    for mask in (inp["mask"], mg):
        ok, why = GO.conditions(inp, mask, delta)
        if not ok:
            return None, why
    out = {f"{name}.in.{k}": v for k, v in inp.items()}
    out[f"{name}.in.mask_gspo"] = mg
    floors = {}
    for variant in GO.VARIANTS:
        mask = mg if variant == "gspo" else inp["mask"]
        for u in (0, 1):
            for m in (0, 1):
                d = delta if m else None
                r32 = ref_run(RG, inp, mask, spec["num_samples"], MAX_GEN[name], variant, bool(u), d, torch.float32)
                r16 = ref_run(RG, inp, mask, spec["num_samples"], MAX_GEN[name], variant, bool(u), d, torch.bfloat16)
                if m:
                    live = (inp["adv"] < 0) & (mask.sum(1) > 0)
                    if bool(r32["opm"].all()) or not bool(r32["opm"].any()) or bool(((r32["mean_kl"][live] - delta).abs() < 1e-3).any()):
                        return None, [f"{variant} u{u}: the off-policy mask is constant or a mean KL sits on delta"]
                key = f"{name}.{variant}.u{u}.m{m}"
                out.update({f"{key}.loss32": r32["loss"], f"{key}.dlogits32": r32["dlogits"], f"{key}.loss16": r16["loss"],
                            f"{key}.policy_ratio": r32["ratio"], f"{key}.kl_div": r32["kl"], f"{key}.opm": r32["opm"]})
                if name == "A":
                    out[f"{key}.dlogits16"] = r16["dlogits"]
                floors[key] = {"loss": GO.rel_l2(r16["loss"], r32["loss"]), "dlogits": GO.rel_l2(r16["dlogits"], r32["dlogits"])}
    return (out, delta, floors), []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    sys.path.insert(0, a.ref)
    from llm_quest.alignment.rlhf_grpo import grpo_engine as RG
    import config as RC

    tensors, meta = {}, {"seeds": {}, "delta": {}, "floors": {}, "scalars": {"min_clip": GO.MIN_CLIP, "max_clip": GO.MAX_CLIP, "beta": GO.BETA},
                         "max_gen": MAX_GEN, "cases": CASES}
    for name, spec in CASES.items():
        for seed in range(64):
            res, why = build_case(RG, name, spec, seed)
            if res is not None:
                break
            print(f"case {name} seed {seed}: {why}")
        else:
            raise SystemExit(f"case {name}: no seed meets the conditions")
        out, delta, floors = res
        tensors.update(out)
        meta["seeds"][name], meta["delta"][name] = seed, delta
        meta["floors"].update(floors)
        print(f"case {name}: seed {seed}, delta {delta:.6f}")

    g = torch.Generator().manual_seed(0)
    rewards = torch.randn(12, generator=g)
    tensors["z.rewards"] = rewards
    for phantom in (0, 1):
        RC.use_phantom_reward = bool(phantom)
        tensors[f"z.p{phantom}.std"] = RG.z_scores(rewards.clone(), 3)
        tensors[f"z.p{phantom}.dr_grpo"] = RG.z_scores(rewards.clone(), 3, dr_grpo="dr_grpo")
    RC.use_phantom_reward = False
    chosen, rejected = torch.randn(7, generator=g), torch.randn(7, generator=g)
    tensors.update({"bt.chosen": chosen, "bt.rejected": rejected, "bt.beta1": RG.bt_loss(chosen, rejected), "bt.beta05": RG.bt_loss(chosen, rejected, beta=0.5)})

    meta["signatures"] = {n: sig(getattr(RG, n)) for n in PUBLIC}
    meta["signatures"].update({f"GRPOLoss.{n}": sig(getattr(RG.GRPOLoss, n)) for n in METHODS})
    from llm_quest_amd.alignment.rlhf_grpo import grpo_engine as OURS

    meta["signatures"]["grpo_policy_loss"] = sig(OURS.grpo_policy_loss)  # this project's own entry: recorded so that it cannot drift unnoticed
    meta["use_phantom_reward_default"] = False
    tensors = {k: (v.to(torch.uint8) if v.dtype == torch.bool else v).contiguous() for k, v in tensors.items()}
    path = os.path.join(a.out, "grpo_tiny.safetensors")
    save_file(tensors, path)
    with open(os.path.join(a.out, "grpo_signatures.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{path}: {os.path.getsize(path)} bytes, {len(tensors)} tensors")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
