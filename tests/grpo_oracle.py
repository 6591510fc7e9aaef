"""Plain-torch restatement of the GRPO loss layer (llm_quest_amd/alignment/rlhf_grpo/grpo_engine.py), written from the mathematics; autograd takes
every derivative.  Each function takes the ``dtype`` all of its arithmetic runs in, which gives the three flows the tests compare:

  * ``torch.float64``: the exact value;
  * ``torch.bfloat16``: the reference's dtype flow -- log-softmax, ratio, KL and the loss all in the logits' bf16;
  * ``torch.float32`` (``own_flow``): the kernels' flow -- fp32 throughout, the logits' gradient rounded to bf16 once at the store.

CPU tensors only; nothing here touches the package under test.
"""

import json
import os

import torch

VARIANTS = ("grpo", "dapo", "dr_grpo", "sapo", "gspo")
TOKEN_LEVEL = VARIANTS[:4]
MIN_CLIP, MAX_CLIP, BETA = 0.2, 0.25, 0.1  # the fixture's scalars (asymmetric clip, so a swapped bound shows)
SAPO_TEMP_POS, SAPO_TEMP_NEG = 1.0, 1.05


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def log_probs_per_token(logits, ids, dtype):
    """log softmax(logits[:, :-1])[ids[:, 1:]] in ``dtype``; (B, S - 1)."""
    x = logits[:, :-1, :].to(dtype)
    return torch.log_softmax(x, dim=-1).gather(-1, ids[:, 1:].unsqueeze(-1)).squeeze(-1)


def lse_per_token(logits, dtype):
    return torch.logsumexp(logits[:, :-1, :].to(dtype), dim=-1)


def log_probs_per_seq(logp, mask):
    m = mask.to(logp.dtype)
    return (logp * m).sum(dim=1) / m.sum(dim=1)


def k3(pol, ref, ratio=None):
    d = ref - pol
    k = torch.exp(d) - d - 1
    return k if ratio is None else ratio * k


def off_policy_mask(kl, adv, mask, delta):
    """(mask bool [B], masked mean KL [B])."""
    m = mask.to(kl.dtype)
    mean = (kl * m).sum(dim=-1) / m.sum(dim=-1).clamp(min=1)
    return (adv >= 0) | (mean <= delta), mean


def clipped_surrogate(ratio, A, min_clip, max_clip):
    return torch.min(ratio * A, torch.clip(ratio, min=1 - min_clip, max=1 + max_clip) * A)


def sapo_surrogate(ratio, A, temp_pos=SAPO_TEMP_POS, temp_neg=SAPO_TEMP_NEG):
    temp = torch.where(A > 0, temp_pos, temp_neg)  # fp32 whatever the flow, as upstream: the bf16 flow's gate is promoted, 1.05 is its fp32 value
    return torch.sigmoid(temp * (ratio - 1)) * 4 / temp * A


def aggregate(loss_per_token, mask, num_samples, max_gen, variant):
    m = mask.to(loss_per_token.dtype)
    if variant in ("grpo", "sapo"):
        per_seq = loss_per_token.sum(dim=-1) / m.sum(dim=-1).clamp(min=1)
        return per_seq.view(-1, num_samples).mean(dim=1).mean()
    if variant == "dapo":
        return loss_per_token.sum() / m.sum().clamp(min=1)
    if variant == "dr_grpo":
        return loss_per_token.sum() / (loss_per_token.shape[0] * max_gen)
    raise ValueError(f"Unknown loss type: {variant}")


def loss_from_logp(pol, old, ref, adv, mask, num_samples, max_gen, variant, unbiased, delta, min_clip=MIN_CLIP, max_clip=MAX_CLIP, beta=BETA):
    """The chain of the training loop from the policy's log-probs, in their dtype.  Returns a dict: loss, ratio (per token, or per sequence for gspo),
    kl (as it enters the loss), opm (bool [B]; all True without ``delta``), mean_kl [B].  For gspo the KL is the plain k3 (a sequence-level ratio does
    not weigh a token's KL) and feeds only the off-policy mask."""
    dt = pol.dtype
    old, ref, adv, m = old.to(dt), ref.to(dt), adv.to(dt), mask.to(dt)
    if variant == "gspo":
        ratio = torch.exp(log_probs_per_seq(pol, mask) - log_probs_per_seq(old, mask))
        kl = k3(pol, ref)
    else:
        ratio = torch.exp(pol - old)
        kl = k3(pol, ref, ratio if unbiased else None)
    opm, mean_kl = off_policy_mask(kl.detach(), adv, mask, delta if delta is not None else 0.0)
    if delta is None:
        opm = torch.ones_like(opm)
    if variant == "gspo":
        loss = (-(clipped_surrogate(ratio, adv, min_clip, max_clip) * opm.to(dt))).mean()
    else:
        A = adv.unsqueeze(-1)
        surr = sapo_surrogate(ratio, A) if variant == "sapo" else clipped_surrogate(ratio, A, min_clip, max_clip)
        surr = surr * opm.to(dt).unsqueeze(-1)
        loss = aggregate(-(surr - beta * kl) * m, mask, num_samples, max_gen, variant)
    return {"loss": loss, "ratio": ratio, "kl": kl, "opm": opm, "mean_kl": mean_kl}


def loss_and_grads(logits, ids, old, ref, adv, mask, num_samples, max_gen, variant, unbiased, delta, dtype, **scalars):
    """From the logits: the dict of ``loss_from_logp`` plus logp (B, S - 1), dlogp = d loss / d logp and dlogits = d loss / d logits (B, S, V; row S - 1
    zero), all in ``dtype``."""
    x = logits.detach().to(dtype).requires_grad_(True)
    logp = log_probs_per_token(x, ids, dtype)
    logp.retain_grad()
    out = loss_from_logp(logp, old, ref, adv, mask, num_samples, max_gen, variant, unbiased, delta, **scalars)
    out["loss"].backward()
    out = {k: v.detach() for k, v in out.items()}
    out.update(logp=logp.detach(), dlogp=logp.grad.detach(), dlogits=x.grad.detach())
    return out


def own_flow(logits, ids, old, ref, adv, mask, num_samples, max_gen, variant, unbiased, delta, **scalars):
    """The kernels' flow: fp32 throughout, the logits' gradient rounded to bf16 once."""
    out = loss_and_grads(logits, ids, old, ref, adv, mask, num_samples, max_gen, variant, unbiased, delta, torch.float32, **scalars)
    out["dlogits"] = out["dlogits"].to(torch.bfloat16)
    return out


def logprob_grad(logits, ids, g, dtype):
    """d (sum g * logp) / d logits in ``dtype``: the label log-prob backward with a weight per token."""
    x = logits.detach().to(dtype).requires_grad_(True)
    (log_probs_per_token(x, ids, dtype) * g.to(dtype)).sum().backward()
    return x.grad.detach()


def z_scores(rewards, num_samples, dr_grpo=None, phantom=False):
    r = rewards.view(-1, num_samples)
    aug = torch.cat([r, torch.zeros(r.shape[0], 1, dtype=r.dtype)], dim=1) if phantom else r
    mean = aug.mean(dim=1, keepdim=True)
    if dr_grpo == "dr_grpo":
        return (r - mean).view(-1)
    return ((r - mean) / (aug.std(dim=1, keepdim=True) + 1e-8)).view(-1)


def bt_loss(chosen, rejected, beta=1.0):
    return -torch.nn.functional.logsigmoid(beta * (chosen - rejected)).mean()


# ------------------------------------------------------------------------------------------------------------- the fixture's inputs
def fixture_inputs(B, S, V, num_samples, seed, dead_seq=None, noise=0.3):
    """bf16 logits 3 N(0, 1), ids, masks that start and end at different positions per sequence (``dead_seq`` masked out entirely), old / reference
    log-probs = the fp64 policy log-probs + ``noise`` N(0, 1), advantages = z-scores of N(0, 1) rewards."""
    g = torch.Generator().manual_seed(seed)
    logits = (3.0 * torch.randn(B, S, V, generator=g)).to(torch.bfloat16)
    ids = torch.randint(0, V, (B, S), generator=g)
    T = S - 1
    mask = torch.zeros(B, T, dtype=torch.bool)
    for b in range(B):
        start = b % max(2, T // 2)
        end = T - ((b // 2) % (T // 3) if T >= 6 else (b + 1) % 2)
        mask[b, start:max(end, start + 1)] = True
    if dead_seq is not None:
        mask[dead_seq] = False
    logp = log_probs_per_token(logits, ids, torch.float64)
    old = (logp + noise * torch.randn(B, T, generator=g, dtype=torch.float64)).float()
    ref = (logp + noise * torch.randn(B, T, generator=g, dtype=torch.float64)).float()
    adv = z_scores(torch.randn(B, generator=g, dtype=torch.float64), num_samples).float()
    return {"logits": logits, "ids": ids, "mask": mask, "old": old, "ref": ref, "adv": adv}


def conditions(inp, mask, delta, min_clip=MIN_CLIP, max_clip=MAX_CLIP):
    """The three conditions a fixture's inputs must meet; returns (ok, reasons).  ``delta`` None: the third is not asked."""
    why = []
    logp = log_probs_per_token(inp["logits"], inp["ids"], torch.float64)
    ratio = torch.exp(logp - inp["old"].double())
    seq = torch.exp(log_probs_per_seq(logp, mask) - log_probs_per_seq(inp["old"].double(), mask))
    for r in (ratio[mask], seq[~torch.isnan(seq)]):
        if bool((((r - (1 - min_clip)).abs() < 1e-3) | ((r - (1 + max_clip)).abs() < 1e-3)).any()):
            why.append("a ratio lies within 1e-3 of a clip bound")
    if bool((inp["adv"] == 0).any()):
        why.append("an advantage is 0")
    if delta is not None:
        opm, _ = off_policy_mask(k3(logp, inp["ref"].double()), inp["adv"].double(), mask, delta)
        if bool(opm.all()) or not bool(opm.any()):
            why.append("the off-policy mask is constant")
    return not why, why


def midway_delta(inp, mask):
    """A threshold midway between two per-sequence mean KLs (plain k3, fp64) such that the off-policy mask holds a True and a False, or None."""
    logp = log_probs_per_token(inp["logits"], inp["ids"], torch.float64)
    _, mean = off_policy_mask(k3(logp, inp["ref"].double()), inp["adv"].double(), mask, 0.0)
    neg = sorted(float(v) for v, a, c in zip(mean, inp["adv"], mask.sum(dim=1)) if a < 0 and c > 0)
    if not neg:
        return None
    lower = max([float(v) for v in mean if float(v) < neg[-1]], default=None)
    return None if lower is None else 0.5 * (lower + neg[-1])


# ------------------------------------------------------------------------------------------------------------- the committed fixture
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_fixture():
    """(tensors of tests/golden/grpo_tiny.safetensors, the dict of grpo_signatures.json)."""
    from safetensors.torch import load_file

    with open(os.path.join(GOLDEN, "grpo_signatures.json")) as f:
        meta = json.load(f)
    return load_file(os.path.join(GOLDEN, "grpo_tiny.safetensors")), meta


def configs():
    """Every (variant, unbiased, off-policy mask) the fixture holds."""
    return [(v, u, m) for v in VARIANTS for u in (0, 1) for m in (0, 1)]


def case_args(t, meta, case, variant, u, m):
    """The positional arguments of ``loss_and_grads`` / ``own_flow`` (without the dtype) for one configuration of a fixture case, and its key."""
    spec = meta["cases"][case]
    mask = t[f"{case}.in.mask_gspo" if variant == "gspo" else f"{case}.in.mask"].bool()
    delta = meta["delta"][case] if m else None
    args = (t[f"{case}.in.logits"], t[f"{case}.in.ids"], t[f"{case}.in.old"], t[f"{case}.in.ref"], t[f"{case}.in.adv"], mask, spec["num_samples"],
            meta["max_gen"][case], variant, bool(u), delta)
    return args, f"{case}.{variant}.u{u}.m{m}"


def loss_and_dlogp(pol, old, ref, adv, mask, num_samples, max_gen, variant, unbiased, delta, dtype, **scalars):
    """``loss_from_logp`` from the policy's log-probs in ``dtype``, plus dlogp = d loss / d pol."""
    p = pol.detach().to(dtype).requires_grad_(True)
    out = loss_from_logp(p, old, ref, adv, mask, num_samples, max_gen, variant, unbiased, delta, **scalars)
    out["loss"].backward()
    out = {k: v.detach() for k, v in out.items()}
    out["dlogp"] = p.grad.detach()
    return out


def synthetic_logp(B, T, seed, noise=0.3, min_clip=MIN_CLIP, max_clip=MAX_CLIP):
    """Log-probs of a long batch under the fixture's conditions: policy = -|2 N(0, 1)| - 0.05, old = policy + ``noise`` N(0, 1), reference = policy + ``noise`` (0.5 + 0.5 b) N(0, 1), with a
    token's old-policy noise drawn again while its fp64 ratio lies within 1e-3 of a clip bound (so no token is excluded), non-zero advantages, every token live
    but ragged ends.  Returns a dict like ``fixture_inputs`` with ``pol`` instead of logits."""
    g = torch.Generator().manual_seed(seed)
    pol = (-(2.0 * torch.randn(B, T, generator=g, dtype=torch.float64)).abs() - 0.05).float()
    old = (pol.double() + noise * torch.randn(B, T, generator=g, dtype=torch.float64)).float()
    for _ in range(64):
        r = torch.exp(pol.double() - old.double())
        bad = ((r - (1 - min_clip)).abs() < 1e-3) | ((r - (1 + max_clip)).abs() < 1e-3)
        if not bool(bad.any()):
            break
        old = torch.where(bad, (pol.double() + noise * torch.randn(B, T, generator=g, dtype=torch.float64)).float(), old)
    spread = noise * (0.5 + 0.5 * torch.arange(B, dtype=torch.float64)).unsqueeze(-1)  # per sequence, so that the mean KLs of long sequences stand apart
    ref = (pol.double() + spread * torch.randn(B, T, generator=g, dtype=torch.float64)).float()
    adv = z_scores(torch.randn(B, generator=g, dtype=torch.float64), 2).float()
    mask = torch.ones(B, T, dtype=torch.bool)
    for b in range(B):
        mask[b, : 3 * b] = False
        mask[b, T - 5 * b:] = False if b else True
    return {"pol": pol, "old": old, "ref": ref, "adv": adv, "mask": mask}
