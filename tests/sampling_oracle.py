"""fp64 restatement of the rollout kernels (csrc/sampling.hip) in NumPy, the Philox4x32-10 generator in pure Python, and the case lists that the
fixture generator (tools/gen_golden_rollout.py) and the tests share.

The sampler's definition (include/mi355_vlm.h: mi355_sample_rows), row by row, vectorised over the rows:
  p = softmax(x / temp) with the row maximum subtracted; every ordering is that of the logits themselves (equal logits are exact ties), descending, the
  lower token index first among equals; the filter is min_p if set and non-zero, else top_p, else top_k, else none; the draw returns the first kept
  token in token-index order whose running kept mass exceeds u * Z.
Besides the kept set and the token, ``sample_oracle`` reports the margins: how far the decisions are from flipping (relative distance of ``top_p`` to the
nearest running sum, of ``min_p * p_max`` to the nearest probability, of ``u * Z`` to the nearest CDF step), and whether a tie straddles the boundary.
"""

import numpy as np
import torch

MASK32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1, PHILOX_W0, PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11): four counter words and two key words -> four output words."""
    c0, c1, c2, c3 = (int(c) & MASK32 for c in counter)
    k0, k1 = (int(k) & MASK32 for k in key)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & MASK32, p1 & MASK32, ((p0 >> 32) ^ c3 ^ k1) & MASK32, p0 & MASK32
        k0, k1 = (k0 + PHILOX_W0) & MASK32, (k1 + PHILOX_W1) & MASK32
    return c0, c1, c2, c3


def philox_uniform(seed, offset, row):
    """The sampler's uniform of a row: key = the seed's low and high words, counter = (row, 0, offset low, offset high), u = (word 0 >> 8) * 2^-24."""
    seed, offset = int(seed) & (2**64 - 1), int(offset) & (2**64 - 1)
    w = philox4x32_10((row, 0, offset & MASK32, offset >> 32), (seed & MASK32, seed >> 32))
    return (w[0] >> 8) * 2.0**-24


def philox_uniforms(seed, offset, rows):
    return np.array([philox_uniform(seed, offset, r) for r in range(rows)], dtype=np.float64)


def as_f64(logits):
    """The exact values of a bf16 / fp32 torch tensor (or an array) as fp64 [B, V]."""
    if isinstance(logits, torch.Tensor):
        logits = logits.detach().cpu().to(torch.float64).numpy()
    x = np.asarray(logits, dtype=np.float64)
    return x[None, :] if x.ndim == 1 else x


def sample_oracle(logits, top_k=None, top_p=None, min_p=None, temp=1.0, u=None):
    """dict of per-row results: ``kept`` bool [B, V], ``probs`` fp64 [B, V] (renormalised over the kept set), ``cdf`` [B, V] (running kept mass over token
    index, divided by Z), ``token`` int64 [B] (with ``u``), ``margin_p`` / ``margin_min_p`` / ``margin_u`` [B] (inf where the mode has no such decision) and
    ``boundary_tie`` bool [B]: a token equal to the last kept one (in the filter's order) is dropped."""
    if top_p is not None and min_p is not None:
        raise ValueError("cannot use top_p and min_p together")
    if not temp > 0:
        raise ValueError("temp must be positive")
    x = as_f64(logits)
    B, V = x.shape
    if top_k and not 1 <= top_k <= V:
        raise ValueError("top_k outside 1..V")
    rows = np.arange(B)[:, None]
    z = x / temp
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    order = np.argsort(-x, axis=1, kind="stable")  # descending value, lower index first among equals
    rank = np.empty_like(order)
    rank[rows, order] = np.arange(V)[None, :]
    xs, ps = np.take_along_axis(x, order, 1), np.take_along_axis(p, order, 1)
    margin_p = np.full(B, np.inf)
    margin_mp = np.full(B, np.inf)
    tie = np.zeros(B, dtype=bool)
    pos = np.arange(V)[None, :]
    if min_p:
        m = top_k if top_k else 1
        thr = min_p * p.max(axis=1, keepdims=True)
        kept = (p >= thr) | (rank < m)
        margin_mp = (np.abs(p - thr) / thr).min(axis=1)
        if m < V:  # a dropped token equal to the m-th in order, which only its place saved
            tie = (xs[:, m - 1] == xs[:, m]) & (ps[:, m - 1] < thr[:, 0])
    elif top_p:
        cand = np.ones((B, V), dtype=bool)
        if top_k:
            cand = xs >= xs[:, top_k - 1 : top_k]  # every tie at the k-th largest value stays a candidate
        ncand = cand.sum(axis=1)
        cum = np.cumsum(ps * cand, axis=1)
        over = (cum > top_p) & cand
        first = np.where(over.any(axis=1), over.argmax(axis=1), ncand - 1)
        kept_sorted = cand & (pos <= first[:, None])
        margin_p = np.where(cand, np.abs(cum - top_p) / top_p, np.inf).min(axis=1)
        nxt = np.minimum(first + 1, V - 1)
        tie = (first + 1 < V) & (xs[rows[:, 0], first] == xs[rows[:, 0], nxt]) & over.any(axis=1)
        kept = np.zeros((B, V), dtype=bool)
        kept[rows, order] = kept_sorted
    elif top_k:
        kept = rank < top_k
        if top_k < V:
            tie = xs[:, top_k - 1] == xs[:, top_k]
    else:
        kept = np.ones((B, V), dtype=bool)
    pk = p * kept
    Z = pk.sum(axis=1)
    c = np.cumsum(pk, axis=1)
    out = {"kept": kept, "probs": pk / Z[:, None], "cdf": c / Z[:, None], "p": p, "Z": Z, "margin_p": margin_p, "margin_min_p": margin_mp, "boundary_tie": tie}
    if u is not None:
        out.update(draw(out, u))
    return out


def draw(info, u):
    """The draw on a finished ``sample_oracle`` result: ``token`` int64 [B] and ``margin_u`` [B] for the uniforms ``u``."""
    kept, pk, Z = info["kept"], info["p"] * info["kept"], info["Z"]
    B, V = kept.shape
    c = np.cumsum(pk, axis=1)
    u = np.broadcast_to(np.asarray(u, dtype=np.float64), (B,))
    target = u * Z
    live = kept & (pk > 0)
    hit = (c > target[:, None]) & live
    last = V - 1 - live[:, ::-1].argmax(axis=1)
    steps = np.where(live, np.abs(c - target[:, None]), np.inf)
    return {"token": np.where(hit.any(axis=1), hit.argmax(axis=1), last).astype(np.int64), "margin_u": steps.min(axis=1) / Z}


def midpoint_uniforms(info, pick=0, min_prob=1e-3):
    """Per row a uniform (fp32-representable) at the midpoint of the CDF interval of a kept token whose renormalised probability is >= ``min_prob``: the
    ``(pick + row) % n``-th such token in token order.  Returns (u fp32 [B], the token of each row)."""
    probs, cdf = info["probs"], info["cdf"]
    B = probs.shape[0]
    u, tok = np.zeros(B, dtype=np.float32), np.zeros(B, dtype=np.int64)
    for b in range(B):
        big = np.nonzero(probs[b] >= min_prob)[0]
        assert len(big) > 0, "no kept token carries 1e-3 of the mass"
        j = big[(pick + b) % len(big)]
        u[b] = np.float32(cdf[b, j] - 0.5 * probs[b, j])
        tok[b] = j
    return u, tok


# ------------------------------------------------------------------------------------------------ the rollout's bookkeeping and the response masks
def rollout_step(sampled, finished, eos_ids, pad_id):
    """(token, finished, mask column) of one generated token: finished rows emit ``pad_id``; ``finished |= token in eos_ids``; the key-mask column is
    ``!finished`` after that update."""
    eos = [eos_ids] if isinstance(eos_ids, int) else list(eos_ids)
    token = np.where(finished, pad_id, sampled)
    finished = finished | np.isin(token, eos)
    return token, finished, ~finished


def response_masks(responses, prompt_masks, eos_ids=50256, pad_token_id=50256):
    """(attn_masks, reward_masks), bool [B, S]: a column >= P is attended while at most one stop token (an EOS id or the pad id, at a column >= P) has
    been seen up to and including it; a prompt column takes ``prompt_masks``; the reward mask is the attention mask without the prompt."""
    r = np.asarray(responses)
    pm = np.asarray(prompt_masks).astype(bool)
    B, S = r.shape
    P = pm.shape[1]
    eos = [eos_ids] if isinstance(eos_ids, int) else list(eos_ids)
    attn = np.zeros((B, S), dtype=bool)
    for b in range(B):
        stops = 0
        for s in range(S):
            if s < P:
                attn[b, s] = pm[b, s]
                continue
            if r[b, s] == pad_token_id or r[b, s] in eos:
                stops += 1
            attn[b, s] = stops <= 1
    reward = attn.copy()
    reward[:, :P] = False
    return attn, reward


# ------------------------------------------------------------------------------------------------ shared case lists
TEMPS = (1e-3, 0.7, 1.0, 1.5)
FIXTURE_VS = (7, 64, 255, 256, 257, 1000, 4099)
ROWS = 2  # base rows per vocabulary size in the fixture


def modes_for(V):
    """The sampler configurations of the grid at vocabulary size V, as (name, kwargs); k is capped at V."""
    out = []
    for k in (1, 2, 20, 64, V):
        k = min(k, V)
        if not any(m[1].get("top_k") == k and len(m[1]) == 1 for m in out):
            out.append((f"k{k}", {"top_k": k}))
    out += [("p0.5", {"top_p": 0.5}), ("p0.9", {"top_p": 0.9}), ("p0.5k20", {"top_p": 0.5, "top_k": min(20, V)}), ("p0.9k20", {"top_p": 0.9, "top_k": min(20, V)}),
            ("m0.1", {"min_p": 0.1}), ("m0.1k5", {"min_p": 0.1, "top_k": min(5, V)}), ("none", {})]
    return out


def fixture_modes(V):
    """The configurations whose reference probabilities the fixture stores: all of them up to V = 1 000, four at V = 4 099 (the file stays small)."""
    ms = modes_for(V)
    return ms if V <= 1000 else [m for m in ms if m[0] in ("k20", "p0.9", "p0.9k20", "m0.1k5")]


def case_temp(V, mode_index):
    """The temperature a fixture case runs at: the four temperatures in turn."""
    return TEMPS[(mode_index + FIXTURE_VS.index(V)) % len(TEMPS)]


def base_rows(V, seed):
    """fp32 N(0, 1) [ROWS, V] of a seed."""
    g = torch.Generator().manual_seed(1000 * V + seed)
    return torch.randn(ROWS, V, generator=g, dtype=torch.float32)


def logits_from_base(base, temp, dtype, spread=3.0):
    """The logits of a case: ``spread`` temp N(0, 1), so that x / temp spans the same range at every temperature (at temp = 1e-3 unscaled logits would leave
    one token with all the mass in fp32 and fp64 alike), rounded to ``dtype``.  ``spread`` 3 up to a few thousand tokens; a row of 151 936 needs 10 to be as
    peaked as a language model's (at 3 its mass lies in a bulk of tokens of 1e-6 each, and no ``top_p`` is 1e-4 away from a running sum)."""
    return (base * (spread * temp)).to(dtype)


def spread_rows(x, B):
    """B rows from the base rows: row j is base row j % ROWS rolled by 37 j places -- the same values, so the same running sums in the filters' order, at
    other token indices."""
    return torch.stack([torch.roll(x[j % x.shape[0]], 37 * j) for j in range(B)])
