"""Generate the rollout fixture by running the REFERENCE on the CPU.  Run from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_rollout.py --ref <path to the reference checkout> [--out tests/golden]

The reference package is imported at run time from ``--ref`` (nothing of it is copied here, and it is never present where the GPU tests run).
Output, tensors and names only:

  * ``rollout_tiny.safetensors`` (well under 1 MiB).
    - ``base.<V>``: fp32 N(0, 1) [2, V] for V in 7, 64, 255, 256, 257, 1 000, 4 099; the logits of a case are ``sampling_oracle.logits_from_base`` of it
      (3 temp N(0, 1) rounded to bf16 or fp32 -- derived, not stored).
    - ``probs.<V>.<mode>``: the reference's filtered, renormalised ``probs`` (the argument its ``sampling`` hands ``torch.multinomial``, captured by wrapping
      that call) on the fp32 values of the case's logits, for every configuration of ``sampling_oracle.fixture_modes(V)``.
    - ``tie.<name>.x``: small rows with a tie exactly at a filter's boundary (the oracle's own definition decides them; the reference is not asked).
    - ``prompts.*`` / ``resp.*``: both collators' outputs on small ragged batches (a prompt that holds the pad id, a response without a stop token, a stop
      token in the first response column, P = 1).
    - ``roll.<scenario>.*``: the transcript of the reference's ``generate_batched_loop_kv_cache`` on a stub model that returns canned logits, its ``sampling``
      replaced by the oracle under scripted uniforms: every call's ``attn_mask`` and ``position_ids``, and the returned tensor.
  * ``rollout_signatures.json``: the seeds, each case's temperature / dtype / floor (largest distance of the reference's fp32 run to its fp64 run), the
    scenarios' scalars, the parameter lists of the reference's and of this project's new public names.

Conditions (not measurements) the sampler inputs must meet; per V the seed is the first of 0, 1, 2, ... that meets them:
  * in every configuration of ``sampling_oracle.modes_for(V)``, at all four temperatures, in bf16 and in fp32 (the grid of the GPU tests): ``top_p`` is at least
    1e-4 (relative) away from every running sum, ``min_p * p_max`` from every probability, and some kept token carries 1e-3 of the kept mass (the scripted
    uniforms sit at the midpoint of such a token's CDF interval);
  * in the stored cases: no tie straddles the filter's boundary, and the reference's kept set (``probs > 0``) equals the oracle's.
"""

import argparse
import inspect
import json
import os
import sys

os.environ.setdefault("HF_HUB_OFFLINE", "1")

import numpy as np
import torch
from safetensors.torch import save_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import sampling_oracle as SO  # noqa: E402

MARGIN = 1e-4
SCENARIOS = {
    # rows finish at different tokens, row 2 never; finish[b] = the generated token at which row b emits an EOS id (None: never)
    "ragged": dict(B=4, P=5, V=50, max_gen=6, lens=[5, 3, 4, 2], finish=[1, 4, None, 0], eos_ids=[7, 9], pad_id=3, seed=0),
    # every row has finished by token 2 of 8: the loop stops there
    "early": dict(B=4, P=4, V=50, max_gen=8, lens=[4, 4, 2, 3], finish=[2, 0, 1, 2], eos_ids=[7], pad_id=3, seed=1),
}
ROLL_SAMPLING = dict(top_k=20, temp=1.0)


def sig(fn):
    return [[n, None if p.default is inspect.Parameter.empty else repr(p.default)] for n, p in inspect.signature(fn).parameters.items()]


def ref_probs(RGEN, x, kw, temp):
    """The tensor the reference's ``sampling`` hands ``torch.multinomial``."""
    got = {}
    orig = torch.multinomial

    def wrapped(probs, num_samples, *a, **k):
        got["probs"] = probs.detach().clone()
        return orig(probs, num_samples, *a, **k)

    torch.multinomial = wrapped
    try:
        RGEN.sampling(x.clone(), temp=temp, **kw)
    finally:
        torch.multinomial = orig
    return got["probs"]


def grid_conditions(V, base):
    """The margins of EVERY configuration, temperature and dtype the GPU tests run on these rows (they assert them again)."""
    for name, kw in SO.modes_for(V):
        for temp in SO.TEMPS:
            for dtype in (torch.bfloat16, torch.float32):
                info = SO.sample_oracle(SO.logits_from_base(base, temp, dtype), temp=temp, **kw)
                if info["margin_p"].min() < MARGIN or info["margin_min_p"].min() < MARGIN:
                    return f"{name} at temp {temp} in {dtype}: a margin below {MARGIN}"
                if (info["probs"].max(axis=1) < 1e-3).any():
                    return f"{name} at temp {temp} in {dtype}: no token carries 1e-3"
    return None


def sampler_cases(RGEN, V):
    for seed in range(256):
        base = SO.base_rows(V, seed)
        out, meta, why = {}, {}, grid_conditions(V, base)
        for mi, (name, kw) in enumerate(SO.fixture_modes(V) if why is None else []):
            temp = SO.case_temp(V, mi)
            dtype = torch.bfloat16 if mi % 2 == 0 else torch.float32
            x = SO.logits_from_base(base, temp, dtype)
            info = SO.sample_oracle(x, temp=temp, **kw)
            p32, p64 = ref_probs(RGEN, x.float(), kw, temp), ref_probs(RGEN, x.double(), kw, temp)
            if info["margin_p"].min() < MARGIN or info["margin_min_p"].min() < MARGIN:
                why = f"{name}: a margin below {MARGIN}"
            elif info["boundary_tie"].any():
                why = f"{name}: a tie at the boundary"
            elif not np.array_equal(info["kept"], (p32 > 0).numpy()) or not np.array_equal(info["kept"], (p64 > 0).numpy()):
                why = f"{name}: the reference keeps another set"
            elif (info["probs"].max(axis=1) < 1e-3).any():
                why = f"{name}: no token carries 1e-3"
            if why:
                break
            out[f"probs.{V}.{name}"] = p32
            meta[f"{V}.{name}"] = {"temp": temp, "dtype": "bf16" if dtype == torch.bfloat16 else "fp32", "kwargs": kw,
                                   "floor": float((p32.double() - p64).abs().max()), "kept": [int(n) for n in info["kept"].sum(axis=1)]}
        if why is None:
            out[f"base.{V}"] = base
            return seed, out, meta
        print(f"V {V} seed {seed}: {why}")
    raise SystemExit(f"V {V}: no seed meets the conditions")


def tie_rows():
    """Rows of 64 logits with a tie exactly at a filter's boundary, values that bf16 and fp32 both hold."""
    g = torch.Generator().manual_seed(7)
    low = -4.0 - torch.rand(64, generator=g).mul(8).round() / 8
    rows = {}
    x = low.clone()  # top-k 3: two clear leaders, then three equal values at places 3..5 (indices 40, 11, 29): index 11 stays
    x[5], x[50] = 3.0, 2.5
    x[40] = x[11] = x[29] = 2.0
    rows["top_k"] = (x, {"top_k": 3})
    rows["top_p_top_k"] = (x.clone(), {"top_p": 0.99, "top_k": 3})  # all three ties at the k-th value stay candidates, and 0.99 keeps them all
    x = low.clone()  # top-p 0.5: four equal leaders carry almost all the mass: the walk crosses 0.5 inside the tie, after the third by index
    x[[9, 20, 33, 60]] = 3.0
    rows["top_p"] = (x, {"top_p": 0.5})
    x = low.clone()  # min-p 0.5 with 2 tokens always kept: the 2nd place is a three-way tie far below the threshold: the lowest index stays
    x[17] = 5.0
    x[[8, 30, 45]] = 0.0
    rows["min_p"] = (x, {"min_p": 0.5, "top_k": 2})
    return rows


class Stub(torch.nn.Module):
    """Returns canned logits: the prefill gives row b its first logits at its last real position, decode call i the logits of token i + 1."""

    def __init__(self, canned, last_real, P):
        super().__init__()
        self.trf_blocks = [None]
        self.canned, self.last_real, self.P = canned, last_real, P
        self.calls = []

    def forward(self, x, attn_mask=None, kv_cache=None, position_ids=None):
        i = len(self.calls)
        self.calls.append({"attn_mask": attn_mask.clone(), "position_ids": None if position_ids is None else position_ids.clone(), "x": x.clone()})
        B, V = self.canned.shape[1:]
        if i == 0:
            out = torch.zeros(B, self.P, V)
            out[torch.arange(B), self.last_real] = self.canned[0]
            return out
        return self.canned[i].unsqueeze(1)


def scripted_uniforms(spec, canned):
    """fp32 [max_gen, B]: the uniform that makes the oracle pick an EOS id at a row's scheduled token and an ordinary token (neither EOS nor pad) elsewhere, at the
    midpoint of that token's CDF interval (probability >= 1e-3)."""
    u = np.zeros((spec["max_gen"], spec["B"]), dtype=np.float32)
    for i in range(spec["max_gen"]):
        info = SO.sample_oracle(canned[i], **ROLL_SAMPLING)
        for b in range(spec["B"]):
            big = [j for j in np.nonzero(info["probs"][b] >= 1e-3)[0] if j != spec["pad_id"]]
            want_eos = spec["finish"][b] == i
            pick = [j for j in big if (j in spec["eos_ids"]) == want_eos]
            assert pick, "the canned logits offer no such token"
            j = pick[(i + b) % len(pick)]
            u[i, b] = np.float32(info["cdf"][b, j] - 0.5 * info["probs"][b, j])
    return u


def transcript(RGEN, name, spec):
    g = torch.Generator().manual_seed(spec["seed"])
    B, P, V, max_gen = spec["B"], spec["P"], spec["V"], spec["max_gen"]
    canned = torch.randn(max_gen, B, V, generator=g) * 2.0
    for e in spec["eos_ids"]:
        canned[:, :, e] += 3.0  # an EOS id is always among the likely tokens
    prompts = torch.randint(10, V, (B, P), generator=g)
    mask = torch.zeros(B, P, dtype=torch.bool)
    for b, n in enumerate(spec["lens"]):
        mask[b, :n] = True
        prompts[b, n:] = spec["pad_id"]
    last_real = torch.tensor([n - 1 for n in spec["lens"]])
    u = scripted_uniforms(spec, canned)
    stub = Stub(canned, last_real, P)
    calls = {"n": 0}

    def oracle_sampling(logits, top_k=None, top_p=None, min_p=None, temp=0.0):
        i = calls["n"]
        calls["n"] += 1
        info = SO.sample_oracle(logits, top_k=top_k, top_p=top_p, min_p=min_p, temp=temp, u=u[i])
        assert info["margin_u"].min() > 1e-4
        return torch.from_numpy(info["token"]).unsqueeze(-1)

    orig = RGEN.sampling
    RGEN.sampling = oracle_sampling
    try:
        out = RGEN.generate_batched_loop_kv_cache(prompts.clone(), stub, max_gen, 64, eos_ids=list(spec["eos_ids"]), pad_id=spec["pad_id"], device=torch.device("cpu"),
                                                  last_real=last_real.clone(), attention_mask=mask.clone(), **ROLL_SAMPLING)
    finally:
        RGEN.sampling = orig
    t = {f"roll.{name}.canned": canned, f"roll.{name}.prompts": prompts, f"roll.{name}.mask": mask, f"roll.{name}.last_real": last_real,
         f"roll.{name}.uniforms": torch.from_numpy(u), f"roll.{name}.out": out}
    for i, c in enumerate(stub.calls):
        t[f"roll.{name}.call{i}.attn_mask"] = c["attn_mask"]
        if c["position_ids"] is not None:
            t[f"roll.{name}.call{i}.position_ids"] = c["position_ids"]
    return t, len(stub.calls), calls["n"]


def collator_cases(RG):
    t, meta = {}, {}
    prompt_sets = {"a": [[5, 6, 7, 8], [9], [3, 3, 4]], "b": [[11, 12, 13, 14, 15, 16], [17, 18]]}
    meta["prompts"] = {k: {"prompts": v, "pad_token_id": 3, "custom_max_length": 4 if k == "b" else None} for k, v in prompt_sets.items()}
    for k, m in meta["prompts"].items():
        out = RG.rlhf_grpo_prompt_collator([list(p) for p in m["prompts"]], pad_token_id=m["pad_token_id"], custom_max_length=m["custom_max_length"])
        for n, v in out.items():
            t[f"prompts.{k}.{n}"] = v
    # responses: pad 3, EOS 7 and 9.  Case "a": P = 4 -- a prompt that holds the pad id as a real token; a response without a stop token; a stop token in the first
    # response column; an ordinary response (EOS, then pad).  Case "b": P = 1.
    resp = {
        "a": (torch.tensor([[3, 3, 4, 3, 10, 11, 7, 3, 3], [5, 6, 8, 4, 10, 11, 12, 13, 14], [9, 3, 3, 3, 7, 3, 3, 3, 3], [5, 6, 7, 8, 10, 9, 3, 3, 3]]),
              torch.tensor([[1, 1, 1, 0], [1, 1, 1, 1], [1, 0, 0, 0], [1, 1, 1, 1]], dtype=torch.bool), [7, 9]),
        "b": (torch.tensor([[5, 10, 7, 3], [6, 3, 3, 3], [8, 10, 11, 12]]), torch.ones(3, 1, dtype=torch.bool), 7),
    }
    meta["responses"] = {k: {"eos_ids": v[2], "pad_token_id": 3} for k, v in resp.items()}
    for k, (r, pm, eos) in resp.items():
        out = RG.batched_responses_collator(r.clone(), pm.clone(), device="cpu", eos_ids=eos, pad_token_id=3)
        t[f"resp.{k}.responses"], t[f"resp.{k}.prompt_masks"] = r, pm
        for n, v in out.items():
            t[f"resp.{k}.{n}"] = v
    return t, meta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    sys.path.insert(0, a.ref)
    from llm_quest import generate as RGEN
    from llm_quest.alignment.rlhf_grpo import grpo_engine as RG

    tensors, meta = {}, {"seeds": {}, "cases": {}, "margin": MARGIN, "scenarios": SCENARIOS, "roll_sampling": ROLL_SAMPLING, "calls": {}}
    for V in SO.FIXTURE_VS:
        seed, out, cases = sampler_cases(RGEN, V)
        tensors.update(out)
        meta["seeds"][str(V)] = seed
        meta["cases"].update(cases)
        print(f"V {V}: seed {seed}, {len(cases)} cases")
    meta["ties"] = {}
    for name, (x, kw) in tie_rows().items():
        tensors[f"tie.{name}.x"] = x
        meta["ties"][name] = kw
    t, m = collator_cases(RG)
    tensors.update(t)
    meta.update(m)
    for name, spec in SCENARIOS.items():
        t, model_calls, sampler_calls = transcript(RGEN, name, spec)
        tensors.update(t)
        meta["calls"][name] = {"model": model_calls, "sampler": sampler_calls}
        print(f"scenario {name}: {model_calls} model calls, {sampler_calls} sampled tokens, returned {tuple(t[f'roll.{name}.out'].shape)}")

    meta["signatures"] = {"reference": {
        "sampling": sig(RGEN.sampling), "generate_batched_loop_kv_cache": sig(RGEN.generate_batched_loop_kv_cache),
        "rlhf_grpo_prompt_collator": sig(RG.rlhf_grpo_prompt_collator), "batched_responses_collator": sig(RG.batched_responses_collator),
        "rlhf_grpo_training_loop": sig(RG.rlhf_grpo_training_loop), "GRPOEvaluator.evaluate": sig(RG.GRPOEvaluator.evaluate),
        "GRPOEvaluator._compute_grpo_metrics": sig(RG.GRPOEvaluator._compute_grpo_metrics)}}
    from llm_quest_amd import generate as OURS

    meta["signatures"]["ours"] = {"SampleRNG": sig(OURS.SampleRNG.__init__), "sample_rows": sig(OURS.sample_rows),
                                  "generate_batched_rollouts": sig(OURS.generate_batched_rollouts)}
    tensors = {k: (v.to(torch.uint8) if v.dtype == torch.bool else v).contiguous() for k, v in tensors.items()}
    path = os.path.join(a.out, "rollout_tiny.safetensors")
    save_file(tensors, path)
    with open(os.path.join(a.out, "rollout_signatures.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{path}: {os.path.getsize(path)} bytes, {len(tensors)} tensors")
    assert os.path.getsize(path) + os.path.getsize(os.path.join(a.out, "rollout_signatures.json")) < 1 << 20


if __name__ == "__main__":
    main()
