"""Plain-torch restatement of the label log-probs from hidden states (llm_quest_amd/kernels_grpo_head.py, csrc/grpo_head.hip), written from the
mathematics.  Two levels:

  * the CHUNKED flow on given logits, parameterised by the dtype its arithmetic runs in: per chunk the maximum and the sum of exp(x - maximum), the
    rescale into the running (m, l) -- a side whose maximum is still -inf is left out --, the finish ``lse = m + log l``, and a chunk's gradient
    ``g (onehot - exp(x - lse))``.  ``torch.float32`` is the kernels' own flow, ``torch.float64`` the exact value;
  * the HEAD-level exact reference: ``h.double() @ W.double().T``, log-softmax, the labels' gather, and autograd for dh and dW; in ``torch.bfloat16``
    the same function is the reference's dtype flow (``F.linear`` and ``log_softmax`` in bf16).

CPU tensors only; nothing here touches the package under test.
"""

import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NEG_INF = float("-inf")


def chunks_of(V, step):
    step = min(step, V)
    return [(c0, min(c0 + step, V)) for c0 in range(0, V, step)]


def chunked_state(logits, ids, chunks, dtype):
    """(m, l, label_logit) over rows s < S - 1 after all ``chunks`` of ``logits`` [B, S, V] have passed, in ``dtype``; a label in no chunk leaves NaN."""
    x = logits[:, :-1].to(dtype)
    lab = ids[:, 1:]
    zero = torch.zeros((), dtype=dtype)
    m = l = None
    label = torch.full(lab.shape, float("nan"), dtype=dtype)
    for i, (c0, c1) in enumerate(chunks):
        xc = x[..., c0:c1]
        cm = xc.max(dim=-1).values
        cs = torch.where(cm == NEG_INF, zero, torch.exp(xc - cm.unsqueeze(-1)).sum(dim=-1))
        if i == 0:
            m, l = cm, cs
        else:
            mn = torch.maximum(m, cm)
            l = torch.where(m == NEG_INF, zero, l * torch.exp(m - mn)) + torch.where(cm == NEG_INF, zero, cs * torch.exp(cm - mn))
            m = mn
        inside = (lab >= c0) & (lab < c1)
        picked = xc.gather(-1, (lab - c0).clamp(0, c1 - c0 - 1).unsqueeze(-1)).squeeze(-1)
        label = torch.where(inside, picked, label)
    return m, l, label


def chunked_logprobs(logits, ids, chunks, dtype):
    """(logp, lse) of the chunked flow in ``dtype``, both [B, S - 1]."""
    m, l, label = chunked_state(logits, ids, chunks, dtype)
    lse = m + torch.log(l)
    return label - lse, lse


def chunk_grad(logits, ids, g, lse, c0, c1, dtype):
    """[B, S, c1 - c0] = g (onehot - exp(x - lse)) on columns [c0, c1) in ``dtype``; row S - 1 zero."""
    B, S, V = logits.shape
    x = logits[:, :-1, c0:c1].to(dtype)
    cols = torch.arange(c0, c1).view(1, 1, -1)
    onehot = (cols == ids[:, 1:].unsqueeze(-1)).to(dtype)
    out = torch.zeros((B, S, c1 - c0), dtype=dtype)
    out[:, :-1] = g.to(dtype).unsqueeze(-1) * (onehot - torch.exp(x - lse.to(dtype).unsqueeze(-1)))
    return out


# ------------------------------------------------------------------------------------------------------------- planted logits for the row kernels
ROW_CASES = [(1, 2, 1, 8), (2, 3, 9, 8), (2, 5, 24, 8), (2, 3, 1000, 128), (3, 4, 1003, 128), (1, 3, 8200, 8192), (2, 3, 512, 1024), (4, 80, 264, 128)]
KINDS = ("first_chunk_inf", "all_but_last_inf", "odd_inf", "max_in_last", "pm120", "equal")
_ROW_CASES = {}


def row_case(B, S, V, step):
    """bf16 logits 3 N(0, 1) [B, S, V] with the special rows (as many of ``KINDS`` as the case has rows and its shape allows, starting at a kind that
    depends on the shape, so that the small cases cover different ones), label sets that put a label on both sides of every chunk border, at 0 and at
    V - 1 (a row with -inf entries keeps a finite label), and the CPU flows of the log-probs.  Computed once per case."""
    key = (B, S, V, step)
    if key in _ROW_CASES:
        return _ROW_CASES[key]
    import grpo_oracle as GO

    gen = torch.Generator().manual_seed(2000 + B + 10 * S + V)
    logits = (3.0 * torch.randn(B, S, V, generator=gen)).to(BF16)
    chunks = chunks_of(V, step)
    T = S - 1
    rows = [(b, s) for b in range(B) for s in range(T)]
    usable = [k for k in KINDS if (V >= 2 or k == "equal") and (len(chunks) >= 2 or k not in ("first_chunk_inf", "all_but_last_inf"))]
    first = (B + S + V) % len(usable)
    kinds = {}
    for (b, s), kind in zip(rows, usable[first:] + usable[:first]):
        kinds[(b, s)] = kind
        if kind == "equal":
            logits[b, s] = 1.5
        elif kind == "pm120":
            logits[b, s] = torch.where(torch.arange(V) % 2 == 0, 120.0, -120.0).to(BF16)
        elif kind == "odd_inf":
            logits[b, s, torch.arange(V) % 2 == 1] = NEG_INF
        elif kind == "first_chunk_inf":
            logits[b, s, : chunks[0][1]] = NEG_INF
        elif kind == "all_but_last_inf":
            logits[b, s, : chunks[-1][0]] = NEG_INF
        elif kind == "max_in_last":
            # above every 3 N(0, 1) draw of these widths, yet close enough that the earlier chunks' rescaled sums still count
            logits[b, s, chunks[-1][0] + (chunks[-1][1] - chunks[-1][0]) // 2] = 16.0
    cands = sorted({0, V - 1} | {c for c0, _ in chunks[1:] for c in (c0 - 1, c0)})

    def finite(kind, c):
        if kind == "odd_inf":
            return c - c % 2
        if kind == "first_chunk_inf":
            return max(c, chunks[0][1])
        if kind == "all_but_last_inf":
            return max(c, chunks[-1][0])
        return c

    sets = []
    for i in range(0, min(len(cands), 4 * len(rows)), len(rows)):
        ids = torch.randint(0, V, (B, S), generator=gen)
        for j, (b, s) in enumerate(rows):
            ids[b, s + 1] = finite(kinds.get((b, s)), cands[(i + j) % len(cands)])
        sets.append(ids)
    ids_all = torch.stack(sets)
    flows = {}
    for name, dt in (("64", F64), ("32", F32)):
        per_set = [chunked_logprobs(logits, ids, chunks, dt) for ids in sets]
        flows["logp" + name] = torch.stack([p for p, _ in per_set])
        flows["lse" + name] = per_set[0][1]
    logp16 = torch.stack([GO.log_probs_per_token(logits, ids, BF16) for ids in sets])
    _ROW_CASES[key] = dict(logits=logits, chunks=chunks, ids_all=ids_all, kinds=kinds, logp16=logp16, lse16=GO.lse_per_token(logits, BF16), **flows)
    return _ROW_CASES[key]


def head_reference(h, w, ids, g, dtype):
    """The head-level flow in ``dtype`` (float64: exact; bfloat16: the reference's ``F.linear`` + ``log_softmax``): a dict of logits, logp (B, S - 1), and
    dh, dw = the gradients of ``sum(g * logp)``."""
    hh = h.detach().to(dtype).requires_grad_(True)
    ww = w.detach().to(dtype).requires_grad_(True)
    logits = torch.nn.functional.linear(hh, ww)
    logp = torch.log_softmax(logits[:, :-1], dim=-1).gather(-1, ids[:, 1:].unsqueeze(-1)).squeeze(-1)
    (logp * g.to(dtype)).sum().backward()
    return {"logits": logits.detach(), "logp": logp.detach(), "dh": hh.grad.detach(), "dw": ww.grad.detach()}


def head_loss_reference(h, w, ids, old, ref, adv, mask, num_samples, max_gen, variant, unbiased, delta, dtype, **scalars):
    """The GRPO loss from the hidden states, head level, in ``dtype``: ``F.linear``, log-softmax, the chain of ``grpo_oracle.loss_from_logp``; a dict of
    loss, logp, dh and dw (autograd takes the derivatives)."""
    import grpo_oracle as GO

    hh = h.detach().to(dtype).requires_grad_(True)
    ww = w.detach().to(dtype).requires_grad_(True)
    logp = GO.log_probs_per_token(torch.nn.functional.linear(hh, ww), ids, dtype)
    out = GO.loss_from_logp(logp, old, ref, adv, mask, num_samples, max_gen, variant, unbiased, delta, **scalars)
    out["loss"].backward()
    return {"loss": out["loss"].detach(), "logp": logp.detach(), "dh": hh.grad.detach(), "dw": ww.grad.detach()}


def own_flow_grads(logits, h, w, ids, g, chunks, dw_dtype=BF16):
    """The kernels' flow from the bf16 ``logits`` the chunk GEMMs wrote: fp32 chunked lse, each chunk's gradient rounded to bf16, dH summed over the
    chunks in fp32 and rounded to bf16 once, dW per chunk rounded to ``dw_dtype``.  Returns a dict of logp, lse, dh, dw."""
    logp, lse = chunked_logprobs(logits, ids, chunks, F32)
    B, S, V = logits.shape
    D = h.shape[-1]
    h2, w2 = h.reshape(B * S, D).float(), w.float()
    acc = torch.zeros((B * S, D), dtype=F32)
    dw = torch.zeros((V, D), dtype=dw_dtype)
    for c0, c1 in chunks:
        d = chunk_grad(logits, ids, g, lse, c0, c1, F32).to(BF16).float().reshape(B * S, c1 - c0)
        acc += d @ w2[c0:c1]
        dw[c0:c1] = (d.t() @ h2).to(dw_dtype)
    return {"logp": logp, "lse": lse, "dh": acc.to(BF16).view(B, S, D), "dw": dw}
