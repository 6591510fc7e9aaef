"""Generate the preference-tuning fixture by running the REFERENCE on the CPU.  Run from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_pref.py --ref <path to the reference checkout> [--out tests/golden]

The reference package is imported at run time from ``--ref`` (nothing of it is copied here, and it is never present where the GPU tests run).  Its
``dataset.py`` needs a tokenizer library at import, so the two collate functions are taken out of that file with ``ast`` and executed with ``torch`` in scope.
Output, tensors and names only:

  * ``pref_tiny.safetensors`` (under 1 MiB).
    DPO cases ``A`` (4 pairs, S = 10, V = 40; prompt lengths 1..4, chosen longer than rejected in pair 0 and shorter in pair 1) and ``B`` (2 pairs, S = 4,
    V = 1000): ``<case>.in.*`` = the reference's ``dpo_collate`` of ragged token lists and bf16 logits of the policy and the reference model for both
    sides; ``<case>.logprobs{32,16}`` / ``.logprobs_nomask{32,16}`` = ``compute_logprobs`` of the four (pol / ref x chosen / rejected) in the reference's fp32
    and bf16 runs; per (beta, label_smoothing) of ``pref_oracle.DPO_CONFIGS`` ``<case>.c<i>.out{32,16}`` (loss, chosen reward, rejected reward) and
    ``.dchosen{32,16}`` / ``.drejected{32,16}``, the gradient of the loss to the policy's logits.
    Reward: ``rw.in.*`` = hidden states [3, 7, 64] in fp32 and bf16, a ``Linear(64, 1)``'s weight and bias, the masks of the reference's
    ``pref_reward_collate`` and the same with sequence 1 emptied, the weights ``g`` of the scalar ``sum_b g[b] score[b]``; ``rw.<smp|hmp|lts>.<bias|nobias>.
    <full|empty>.{score,dh,dw,db}{32,16}`` = the three methods (``smp``: ``scores_mean_pooling`` of the head's per-token output) and their gradients.
    Collates: ``col.<i>.{dpo,rm}.*`` = the full output of both collates on three batches (plain; cut by ``allowed_max_length``; for ``dpo_collate``
    ``mask_prompt_tokens=False``); the token lists are in the JSON.
  * ``pref_signatures.json``: parameter names and defaults of every public name, the seeds, the token lists, the measured floors (distance of the
    reference's bf16 run to its fp32 run).

Conditions (not measurements) the inputs must meet; per case the seed is the first of 0, 1, 2, ... that meets them, and it is stored: ``|beta l| < 20`` in every
configuration; every mask sum positive except in the designated empty sequence; no two pairs of a case with equal chosen or equal rejected lengths.
"""

import argparse
import ast
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
import pref_oracle as PO  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32
COLLATE_KW = ({}, {"allowed_max_length": 6}, {})  # the three collate batches; the third has mask_prompt_tokens=False in dpo_collate


def sig(fn):
    return [[n, None if p.default is inspect.Parameter.empty else repr(p.default)] for n, p in inspect.signature(fn).parameters.items()]


def reference_collates(ref):
    """``dpo_collate`` and ``pref_reward_collate`` of the reference's dataset.py, compiled from their own source at run time."""
    path = os.path.join(ref, "llm_quest", "dataset.py")
    tree = ast.parse(open(path).read(), filename=path)
    wanted = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("dpo_collate", "pref_reward_collate")]
    assert len(wanted) == 2, "the reference's dataset.py no longer defines both collate functions"
    scope = {"torch": torch}
    exec(compile(ast.Module(body=wanted, type_ignores=[]), path, "exec"), scope)
    return scope["dpo_collate"], scope["pref_reward_collate"]


def ref_dpo_run(DPOLoss, inp, batch, beta, ls, dtype, masked=True):
    mod = DPOLoss(beta=beta, label_smoothing=ls)
    lg = {n: inp[f"{n}_logits"].to(dtype).clone().requires_grad_(n.startswith("pol")) for n in ("pol_chosen", "pol_rejected", "ref_chosen", "ref_rejected")}
    lp = {n: mod.compute_logprobs(x, batch[n.split("_")[1]], batch[n.split("_")[1] + "_mask"] if masked else None) for n, x in lg.items()}
    loss, cr, rr = mod.compute_loss(lp["pol_chosen"], lp["pol_rejected"], lp["ref_chosen"].detach(), lp["ref_rejected"].detach())
    loss.backward()
    return {"logprobs": torch.stack([lp[n].detach() for n in ("pol_chosen", "pol_rejected", "ref_chosen", "ref_rejected")]),
            "out": torch.stack([loss.detach(), cr, rr]), "dchosen": lg["pol_chosen"].grad, "drejected": lg["pol_rejected"].grad}


def build_dpo(DPOLoss, dpo_collate, name, seed):
    spec = PO.DPO_CASES[name]
    pairs, inp = PO.dpo_inputs(name, seed)
    batch = dpo_collate(pairs, pad_token_id=PO.PAD)
    if tuple(batch["chosen"].shape) != (spec["b"], spec["S"]):
        return None, f"the collate gave {tuple(batch['chosen'].shape)}"
    if len(set(spec["chosen"])) != spec["b"] or len(set(spec["rejected"])) != spec["b"]:
        return None, "two pairs have equal lengths"
    if not bool((batch["chosen_mask"].sum(1) > 0).all() and (batch["rejected_mask"].sum(1) > 0).all()):
        return None, "an empty mask"
    out = {f"{name}.in.{k}": v for k, v in {**batch, **inp}.items()}
    floors = {}
    for tag, masked in (("logprobs", True), ("logprobs_nomask", False)):
        r32, r16 = (ref_dpo_run(DPOLoss, inp, batch, 0.1, 0.0, dt, masked) for dt in (F32, BF16))
        out[f"{name}.{tag}32"], out[f"{name}.{tag}16"] = r32["logprobs"], r16["logprobs"]
        floors[f"{name}.{tag}"] = PO.rel_l2(r16["logprobs"], r32["logprobs"])
    for i, (beta, ls) in enumerate(PO.DPO_CONFIGS):
        r32, r16 = (ref_dpo_run(DPOLoss, inp, batch, beta, ls, dt) for dt in (F32, BF16))
        lp = r32["logprobs"].double()
        if float((beta * ((lp[0] - lp[2]) - (lp[1] - lp[3]))).abs().max()) >= 20:
            return None, f"|beta l| >= 20 at {(beta, ls)}"
        for k in ("out", "dchosen", "drejected"):
            out[f"{name}.c{i}.{k}32"], out[f"{name}.c{i}.{k}16"] = r32[k], r16[k]
            floors[f"{name}.c{i}.{k}"] = PO.rel_l2(r16[k], r32[k])
    return (out, floors, pairs), ""


def build_reward(RG, pref_reward_collate, seed):
    pairs, inp = PO.reward_inputs(seed)
    batch = pref_reward_collate(pairs, pad_token_id=PO.PAD)
    spec = PO.REWARD
    if tuple(batch["chosen"].shape) != (spec["b"], spec["S"]) or not bool((batch["chosen_mask"].sum(1) > 0).all()):
        return None, "the collate's shape or an empty mask"
    full = {"mask": batch["chosen_mask"], "attn": batch["chosen_attn_mask"]}
    empty = {k: v.clone() for k, v in full.items()}
    for v in empty.values():
        v[spec["empty_seq"]] = False
    out = {f"rw.in.{k}": v for k, v in inp.items()}
    out.update({f"rw.in.{k}_full": v for k, v in full.items()})
    out.update({f"rw.in.{k}_empty": v for k, v in empty.items()})
    floors = {}
    calc = RG.PrefRewardCalculator
    for head_tag, with_bias in (("bias", True), ("nobias", False)):
        for mask_tag, masks in (("full", full), ("empty", empty)):
            for kind in PO.POOLINGS:
                runs = {}
                for dt, h in ((F32, inp["h32"]), (BF16, inp["h16"])):
                    head = torch.nn.Linear(spec["E"], 1, bias=with_bias)
                    with torch.no_grad():
                        head.weight.copy_(inp["w"])
                        if with_bias:
                            head.bias.copy_(inp["bias"])
                    head = head.to(dt)
                    x = h.clone().requires_grad_(True)
                    if kind == "smp":
                        score = calc.scores_mean_pooling(head(x), masks["mask"])
                    elif kind == "hmp":
                        score = calc.hidden_states_mean_pooling(x, masks["mask"], head)
                    else:
                        score = calc.last_token_score(x, masks["attn"], head)
                    (score * inp["g"].to(dt)).sum().backward()
                    runs[dt] = {"score": score.detach(), "dh": x.grad, "dw": head.weight.grad, **({"db": head.bias.grad} if with_bias else {})}
                key = f"rw.{kind}.{head_tag}.{mask_tag}"
                for k in runs[F32]:
                    out[f"{key}.{k}32"], out[f"{key}.{k}16"] = runs[F32][k], runs[BF16][k]
                    floors[f"{key}.{k}"] = PO.rel_l2(runs[BF16][k], runs[F32][k])
    return (out, floors, pairs), ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    sys.path.insert(0, a.ref)
    from llm_quest.alignment.dpo import dpo as RD
    from llm_quest.alignment.rlhf_grpo import grpo_engine as RG
    from llm_quest.utils import CheckpointEvaluator
    import config as RC

    dpo_collate, pref_reward_collate = reference_collates(a.ref)
    tensors, meta = {}, {"seeds": {}, "floors": {}, "pairs": {}, "dpo_cases": PO.DPO_CASES, "reward": PO.REWARD, "dpo_configs": PO.DPO_CONFIGS}
    builders = [(n, lambda s, n=n: build_dpo(RD.DPOLoss, dpo_collate, n, s)) for n in PO.DPO_CASES] + [("rw", lambda s: build_reward(RG, pref_reward_collate, s))]
    for name, build in builders:
        for seed in range(64):
            res, why = build(seed)
            if res is not None:
                break
            print(f"case {name} seed {seed}: {why}")
        else:
            raise SystemExit(f"case {name}: no seed meets the conditions")
        out, floors, pairs = res
        tensors.update(out)
        meta["seeds"][name], meta["pairs"][name] = seed, pairs
        meta["floors"].update(floors)
        print(f"case {name}: seed {seed}")

    # the collates on three batches: case A's pairs, plain / cut / with the prompt left unmasked
    pairs = meta["pairs"]["A"]
    for i, kw in enumerate(COLLATE_KW):
        dpo_kw = dict(kw, mask_prompt_tokens=False) if i == 2 else kw
        for k, v in dpo_collate(pairs, pad_token_id=PO.PAD, **dpo_kw).items():
            tensors[f"col.{i}.dpo.{k}"] = v
        for k, v in pref_reward_collate(pairs, pad_token_id=PO.PAD, **kw).items():
            tensors[f"col.{i}.rm.{k}"] = v
    meta["collate_kwargs"] = [dict(kw) for kw in COLLATE_KW]

    meta["signatures"] = {f"DPOLoss.{n}": sig(getattr(RD.DPOLoss, n)) for n in ("__init__", "compute_logprobs", "compute_loss", "forward")}
    meta["signatures"].update({f"DPOEvaluator.{n}": sig(getattr(RD.DPOEvaluator, n)) for n in ("__init__", "_compute_dpo_loss_loader", "evaluate")})
    meta["signatures"]["dpo_training_eval_loop_simple"] = sig(RD.dpo_training_eval_loop_simple)
    meta["signatures"].update({f"PrefRewardCalculator.{n}": sig(getattr(RG.PrefRewardCalculator, n))
                               for n in ("scores_mean_pooling", "hidden_states_mean_pooling", "last_token_score")})
    meta["signatures"].update({n: sig(getattr(RG, n)) for n in ("evaluate_reward_model", "reward_model_training_eval_loop_simple")})
    meta["signatures"].update({f"CheckpointEvaluator.{n}": sig(getattr(CheckpointEvaluator, n))
                               for n in ("__init__", "is_rlhf_grpo_best", "is_rm_accu_best", "is_rlvr_grpo_best")})
    meta["signatures"].update({"dpo_collate": sig(dpo_collate), "pref_reward_collate": sig(pref_reward_collate)})
    from llm_quest_amd.alignment.dpo import dpo as OD
    from llm_quest_amd.alignment.rlhf_grpo import grpo_engine as OG

    # this project's own two names: recorded so that they cannot drift unnoticed
    meta["signatures"]["DPOLoss.forward_from_hidden"] = sig(OD.DPOLoss.forward_from_hidden)
    meta["signatures"]["PrefRewardCalculator.scores_mean_pooling_from_hidden"] = sig(OG.PrefRewardCalculator.scores_mean_pooling_from_hidden)
    meta["rlhf_grpo_checkpoint_dir_tail"] = list(RC.rlhf_grpo_checkpoint_dir.parts[-2:])

    tensors = {k: (v.to(torch.uint8) if v.dtype == torch.bool else v).detach().contiguous() for k, v in tensors.items()}
    path = os.path.join(a.out, "pref_tiny.safetensors")
    save_file(tensors, path)
    with open(os.path.join(a.out, "pref_signatures.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{path}: {os.path.getsize(path)} bytes, {len(tensors)} tensors")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
