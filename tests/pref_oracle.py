"""Plain-torch restatement of preference tuning (llm_quest_amd/alignment/dpo/dpo.py, ``PrefRewardCalculator`` of grpo_engine.py and the kernels of
csrc/preference.hip), written from the mathematics; autograd takes every derivative.  Each function takes the ``dtype`` all of its arithmetic runs in:

  * ``torch.float64``: the exact value;
  * ``torch.bfloat16``: the reference's dtype flow -- log-softmax, the masked average, the head and the pooling all in bf16;
  * ``torch.float32``: the flow of the reference's fp32 run.

Also the generators of the fixture's inputs (shared with tools/gen_golden_pref.py, so that a test can regenerate them from the stored seed) and
``load_fixture``.  CPU tensors only; nothing here touches the package under test.
"""

import json
import os

import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DPO_CONFIGS = ((0.1, 0.0), (0.1, 0.1), (1.0, 0.0))  # (beta, label_smoothing)
PAD = 0
POOLINGS = ("smp", "hmp", "lts")  # scores mean (through the head), hidden-state mean, last token


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ----------------------------------------------------------------------------------------------------------------- DPO
def label_log_probs(logits, ids, dtype):
    return torch.log_softmax(logits[:, :-1, :].to(dtype), dim=-1).gather(-1, ids[:, 1:].unsqueeze(-1)).squeeze(-1)


def seq_average(logp, mask=None):
    """sum_t logp[b, t] mask[b, t + 1] / sum_s mask[b, s] in ``logp``'s dtype (an all-zero mask: NaN); without a mask the mean over the labels."""
    if mask is None:
        return logp.mean(-1)
    m = mask.to(logp.dtype)
    return (logp * m[:, 1:]).sum(-1) / m.sum(-1)


def compute_logprobs(logits, ids, mask, dtype):
    return seq_average(label_log_probs(logits, ids, dtype), mask)


def dpo_loss(pc, pr, rc, rr, beta, ls):
    """(loss, mean chosen reward, mean rejected reward) in the operands' dtype; the rewards are detached and not scaled by beta."""
    c, r = pc - rc, pr - rr
    x = beta * (c - r)
    losses = -F.logsigmoid(x) * (1 - ls) - F.logsigmoid(-x) * ls
    return losses.mean(), c.detach().mean(), r.detach().mean()


def dpo_run(t, case, beta, ls, dtype, masked=True):
    """The whole chain of a fixture case in ``dtype`` from its four logits tensors; returns the four averages, the three outputs and the gradients of
    the loss with respect to the two policy logits."""
    ids = {k: t[f"{case}.in.{k}"] for k in ("chosen", "rejected")}
    masks = {k: (t[f"{case}.in.{k}_mask"].bool() if masked else None) for k in ids}
    lg = {f"{m}_{k}": t[f"{case}.in.{m}_{k}_logits"].to(dtype).clone().requires_grad_(m == "pol") for m in ("pol", "ref") for k in ids}
    lp = {n: compute_logprobs(x, ids[n.split("_")[1]], masks[n.split("_")[1]], dtype) for n, x in lg.items()}
    loss, cr, rr = dpo_loss(lp["pol_chosen"], lp["pol_rejected"], lp["ref_chosen"].detach(), lp["ref_rejected"].detach(), beta, ls)
    loss.backward()
    return {"logprobs": torch.stack([lp[n].detach() for n in ("pol_chosen", "pol_rejected", "ref_chosen", "ref_rejected")]),
            "out": torch.stack([loss.detach(), cr, rr]), "dchosen": lg["pol_chosen"].grad, "drejected": lg["pol_rejected"].grad}


# ----------------------------------------------------------------------------------------------------------------- reward pooling
def _head(x, w, b):
    y = x @ w.reshape(-1)
    return y if b is None else y + b.reshape(())


def scores_mean(rewards, mask):
    """rewards (b, s, 1) or (b, s)."""
    r = rewards.reshape(mask.shape)
    m = mask.to(r.dtype)
    return (r * m).sum(1) / m.sum(1).clamp(min=1)


def hidden_mean(h, mask, w, b):
    m = mask.to(h.dtype)
    pooled = (h * m.unsqueeze(-1)).sum(1) / m.sum(1).clamp(min=1).unsqueeze(-1)
    return _head(pooled, w, b)


def last_token(h, mask, w, b):
    idx = mask.to(torch.int64).sum(-1) - 1  # -1 selects the last row, as torch indexing does
    return _head(h[torch.arange(h.shape[0]), idx], w, b)


def scores_from_hidden(h, mask, w, b):
    return scores_mean(_head(h, w, b), mask)


POOL_FN = {"smp": scores_from_hidden, "hmp": hidden_mean, "lts": last_token}


def pool_run(kind, h, mask, w, b, g, dtype):
    """One pooling in ``dtype`` with the loss ``sum_b g[b] score[b]``: the scores and the gradients of hidden states, weight and bias (None without)."""
    h = h.to(dtype).clone().requires_grad_(True)
    w = w.to(dtype).clone().requires_grad_(True)
    b = None if b is None else b.to(dtype).clone().requires_grad_(True)
    score = POOL_FN[kind](h, mask, w, b)
    (score * g.to(dtype)).sum().backward()
    return {"score": score.detach(), "dh": h.grad, "dw": w.grad, "db": None if b is None else b.grad}


# ----------------------------------------------------------------------------------------------------------------- the fixture's inputs
DPO_CASES = {"A": dict(b=4, S=10, V=40, prompt=(1, 2, 3, 4), chosen=(9, 5, 7, 6), rejected=(6, 8, 4, 9)),  # pair 0: chosen longer; pair 1: rejected longer
             "B": dict(b=2, S=4, V=1000, prompt=(1, 1), chosen=(3, 2), rejected=(2, 3))}
REWARD = dict(b=3, S=7, E=64, prompt=(2, 1, 3), chosen=(6, 4, 5), rejected=(3, 6, 4), empty_seq=1)


def token_lists(spec, V, gen):
    """Ragged preference pairs: a shared prompt, then different responses; token ids in [1, V) (0 pads)."""
    out = []
    for p, c, r in zip(spec["prompt"], spec["chosen"], spec["rejected"]):
        prompt = torch.randint(1, V, (p,), generator=gen).tolist()
        out.append({"prompt": prompt, "chosen": prompt + torch.randint(1, V, (c - p,), generator=gen).tolist(),
                    "rejected": prompt + torch.randint(1, V, (r - p,), generator=gen).tolist()})
    return out


def dpo_inputs(name, seed):
    """Token lists and the four bf16 logits tensors of a DPO case: N(0, 1) * 2 for the policy, the policy's plus N(0, 1) * 0.5 for the reference model."""
    spec = DPO_CASES[name]
    gen = torch.Generator().manual_seed(seed)
    pairs = token_lists(spec, spec["V"], gen)
    shape = (spec["b"], spec["S"], spec["V"])
    out = {}
    for k in ("chosen", "rejected"):
        pol = 2.0 * torch.randn(shape, generator=gen)
        out[f"pol_{k}_logits"] = pol.to(BF16)
        out[f"ref_{k}_logits"] = (pol + 0.5 * torch.randn(shape, generator=gen)).to(BF16)
    return pairs, out


def reward_inputs(seed):
    gen = torch.Generator().manual_seed(seed)
    pairs = token_lists(REWARD, 50, gen)
    b, S, E = REWARD["b"], REWARD["S"], REWARD["E"]
    h = torch.randn((b, S, E), generator=gen)
    return pairs, {"h32": h, "h16": h.to(BF16), "w": torch.randn((1, E), generator=gen) / E ** 0.5, "bias": torch.randn((1,), generator=gen),
                   "g": torch.randn((b,), generator=gen)}


def load_fixture():
    """(tensors, meta) of tests/golden/pref_tiny.safetensors and pref_signatures.json."""
    from safetensors.torch import load_file

    with open(os.path.join(GOLDEN, "pref_signatures.json")) as f:
        meta = json.load(f)
    return load_file(os.path.join(GOLDEN, "pref_tiny.safetensors")), meta
