"""Text generation loops -- API of ``llm_quest/generate.py`` for the paths on SURVEY.md section 8 row f4: ``generate_loop``
(full re-forward per token), ``generate_loop_kv_cache`` (prefill + one-token decode steps through ``KVCache``) and ``sampling``.

Greedy sampling (``temp == 0``, the default) is a HIP kernel (first index of the row maximum).  Stochastic sampling (temperature /
top-k / top-p / min-p) in ``sampling`` and the loops built on it is control logic on a (batch, vocab) tensor per generated token, outside the measured
path: it is restated here with torch device ops so the loops are complete, and says so.

Rollouts are the measured path of an RL step, and have kernels of their own (csrc/sampling.hip; this project's names): ``sample_rows`` draws one token per
row in one launch -- temperature, top-k (any k), top-p, min-p, uniforms from ``SampleRNG``'s Philox stream or handed in -- and ``generate_batched_rollouts``
is the right-padded batched loop on it: the response and key-mask buffers are allocated once, the sampler's launch also does the loop's per-token
bookkeeping, and the host reads four bytes when a sync is due.  ``sampling`` keeps its torch path and torch's random stream.
"""

import torch

from . import kernels_sample as KS
from . import ops_decode
from .utils import KVCache


def _top_k(probs, k):
    top, idx = torch.topk(probs, k)
    return torch.zeros_like(probs).scatter_(-1, idx, top)


def _top_p(probs, p, top_k=None):
    if top_k:
        kth = torch.topk(probs, top_k)[0][..., -1].unsqueeze(-1)
        probs = probs.masked_fill(probs < kth, 0.0)
    sp, idx = torch.sort(probs, dim=-1, descending=True)
    mask = torch.cumsum(sp, dim=-1) > p
    mask[..., 1:] = mask[..., :-1].clone()
    mask[..., 0] = False
    return torch.zeros_like(probs).scatter_(-1, idx, sp.masked_fill(mask, 0.0))


def _min_p(probs, min_p, min_tokens_to_keep=1):
    remove = probs < min_p * torch.amax(probs, dim=-1, keepdim=True)
    keep_idx = torch.topk(probs, min_tokens_to_keep)[1]
    remove.scatter_(-1, keep_idx, False)
    return probs.masked_fill(remove, 0.0)


def sampling(logits, top_k=None, top_p=None, min_p=None, temp=0.0):
    """logits (b, v) -> next token ids (b, 1) (reference: generate.py:472-514)."""
    assert top_p is None or min_p is None, "Cannot use top_p and min_p together"
    if temp == 0.0:
        return ops_decode.argmax_rows(logits if logits.stride(-1) == 1 else logits.contiguous()).unsqueeze(-1)
    probs = torch.softmax(logits.float() / temp, dim=-1)
    if min_p:
        probs = _min_p(probs, min_p, 1 if top_k is None else top_k)
    elif top_p:
        probs = _top_p(probs, top_p, top_k)
    elif top_k:
        probs = _top_k(probs, top_k)
    probs = probs / probs.sum(dim=-1, keepdim=True)
    return torch.multinomial(probs, num_samples=1)


def generate_loop(input_tensor, model, max_gen, context_length, top_k=None, top_p=None, min_p=None, temp=0.0, eos_ids=None, device=torch.device("cuda")):
    """Re-runs the model on the growing sequence for every token (reference: generate.py:29-94)."""
    input_tensor = input_tensor.to(device)
    eos = None
    if eos_ids is not None:
        eos = torch.tensor(eos_ids if isinstance(eos_ids, list) else [eos_ids], device=device, dtype=torch.long)
    for _ in range(max_gen):
        with torch.inference_mode():
            logits = model(input_tensor[:, -context_length:])[:, -1, :]
        next_token = sampling(logits, top_k, top_p, min_p, temp)
        if eos is not None and torch.isin(next_token, eos).any():
            break
        input_tensor = torch.cat((input_tensor, next_token), dim=-1)
    return input_tensor


def generate_loop_kv_cache(input_tensor, model, max_gen, context_length, top_k=None, top_p=None, min_p=None, temp=0.0, eos_ids=None,
                           device=torch.device("cuda"), use_graph=True):
    """Prefill once, then one-token decode steps through the KV cache (reference: generate.py:97-151).  Greedy decoding
    (``temp == 0``) replays one captured hipGraph per token (``use_graph``); sampling runs the steps eagerly."""
    if use_graph and temp == 0.0 and max_gen > 0 and hasattr(model, "trf_blocks") and input_tensor.shape[-1] + max_gen <= context_length:
        return _generate_greedy_graph(input_tensor, model, max_gen, context_length, eos_ids, device)
    token_ids = []
    kv_cache = KVCache(num_layers=len(model.trf_blocks), prompt_len=input_tensor.shape[-1], context_len=context_length)
    input_tensor = input_tensor.to(device)
    eos = None
    if eos_ids is not None:
        eos = torch.tensor(eos_ids if isinstance(eos_ids, list) else [eos_ids], device=device, dtype=torch.long)
    trunc_input = input_tensor[:, -context_length:]
    next_position_id = torch.tensor([[trunc_input.shape[-1]]], dtype=torch.long, device=device)
    with torch.inference_mode():
        logits = model(trunc_input, kv_cache=kv_cache)[:, -1, :]
        for _ in range(max_gen):
            next_token = sampling(logits, top_k, top_p, min_p, temp)
            if eos is not None and torch.isin(next_token, eos).any():
                break
            token_ids.append(next_token)
            logits = model(next_token, kv_cache=kv_cache, position_ids=next_position_id).squeeze(1)
            next_position_id += 1
    return torch.cat([input_tensor] + token_ids, dim=-1)


def _generate_greedy_graph(input_tensor, model, max_gen, context_length, eos_ids, device):
    token_ids = []
    kv_cache = KVCache(num_layers=len(model.trf_blocks), prompt_len=input_tensor.shape[-1], context_len=context_length)
    input_tensor = input_tensor.to(device)
    eos = None
    if eos_ids is not None:
        eos = torch.tensor(eos_ids if isinstance(eos_ids, list) else [eos_ids], device=device, dtype=torch.long)
    with torch.inference_mode():
        logits = model(input_tensor[:, -context_length:], kv_cache=kv_cache)[:, -1, :]
        next_token = sampling(logits)
        dec = None
        try:
            for _ in range(max_gen):
                if eos is not None and torch.isin(next_token, eos).any():
                    break
                token_ids.append(next_token)
                if len(token_ids) == max_gen:
                    break
                if dec is None:
                    dec = ops_decode.GraphDecoder(model, kv_cache, next_token, max_gen)
                next_token = dec.step()
        finally:
            if dec is not None:
                dec.close()
    return torch.cat([input_tensor] + token_ids, dim=-1)


def _batched_kv_loop(input_tensor, model, max_gen, context_length, top_k, top_p, min_p, temp, eos_ids, pad_id, device, attention_mask,
                     first_position_ids, next_pos_ids, pick_first_logits):
    """Shared body of the two padded, batched KV-cache loops: prefill, then one token per unfinished sequence; finished sequences keep
    receiving ``pad_id`` and are masked out of later attention (reference: generate.py:252-365, 368-469)."""
    input_tensor = input_tensor.to(device)
    attention_mask = attention_mask.bool().to(device)
    eos = torch.tensor(eos_ids if isinstance(eos_ids, list) else [eos_ids], device=device, dtype=torch.long)
    pad = torch.tensor(pad_id, device=device, dtype=torch.long)
    finished = torch.zeros(input_tensor.shape[0], dtype=torch.bool, device=device)
    kv_cache = KVCache(num_layers=len(model.trf_blocks), prompt_len=input_tensor.shape[-1], context_len=context_length)
    generated = []
    with torch.inference_mode():
        logits = pick_first_logits(model(input_tensor, attn_mask=attention_mask, kv_cache=kv_cache, position_ids=first_position_ids))
        for i in range(max_gen):
            next_token = torch.where(finished.unsqueeze(-1), pad, sampling(logits, top_k, top_p, min_p, temp))
            generated.append(next_token)
            finished |= torch.isin(next_token.squeeze(1), eos)
            attention_mask = torch.cat([attention_mask, (~finished).unsqueeze(-1)], dim=-1)
            if finished.all():
                break
            if i < max_gen - 1:
                logits = model(next_token, attn_mask=attention_mask, kv_cache=kv_cache, position_ids=next_pos_ids).squeeze(1)
            next_pos_ids = next_pos_ids + 1
    return torch.cat([input_tensor] + generated, dim=1)


def generate_batched_loop_kv_cache(input_tensor, model, max_gen, context_length, top_k=None, top_p=None, min_p=None, temp=0.0, eos_ids=50256,
                                   pad_id=50256, device=torch.device("cuda"), last_real=None, *, attention_mask):
    """RIGHT-padded prompts: the first logits come from each sequence's last real token, rotary positions continue from its real
    length (reference: generate.py:252-365)."""
    attention_mask = attention_mask.bool().to(device)
    if last_real is not None:
        last_real = last_real.to(device)
        next_pos = last_real.unsqueeze(-1) + 1
    else:
        next_pos = attention_mask.sum(dim=-1, keepdim=True)
        last_real = next_pos.squeeze(-1) - 1
    rows = torch.arange(input_tensor.shape[0], device=device)
    return _batched_kv_loop(input_tensor, model, max_gen, context_length, top_k, top_p, min_p, temp, eos_ids, pad_id, device, attention_mask,
                            None, next_pos, lambda lg: lg[rows, last_real, :])


def generate_batched_loop_kv_cache_left_pad(input_tensor, model, max_gen, context_length, top_k=None, top_p=None, min_p=None, temp=0.0,
                                            eos_ids=50256, pad_id=50256, device=torch.device("cuda"), *, attention_mask):
    """LEFT-padded prompts: positions count real tokens only (pads sit at position 0), every sequence ends in the last column
    (reference: generate.py:368-469)."""
    attention_mask = attention_mask.bool().to(device)
    position_ids = (attention_mask.cumsum(dim=-1) - 1).masked_fill(~attention_mask, 0)
    next_pos = attention_mask.sum(dim=-1, keepdim=True)
    return _batched_kv_loop(input_tensor, model, max_gen, context_length, top_k, top_p, min_p, temp, eos_ids, pad_id, device, attention_mask,
                            position_ids, next_pos, lambda lg: lg[:, -1, :])


# ------------------------------------------------------------------------------------------------ rollouts on the sampling kernels (csrc/sampling.hip)
class SampleRNG:
    """The counter-based random stream of ``sample_rows``: Philox4x32-10 keyed by ``seed`` (default ``torch.initial_seed()``), the counter holding the row
    and ``offset``.  The offset lives on the host, grows by one per sampling call and is never read from the device; a row's uniform depends on (seed,
    offset, row) alone -- not on the batch size."""

    def __init__(self, seed=None):
        self.seed = int(torch.initial_seed() if seed is None else seed) & (2**64 - 1)
        self.offset = 0

    def advance(self):
        offset = self.offset
        self.offset += 1
        return offset


_default_rng = None


def _rng_or_default(rng):
    global _default_rng
    if rng is not None:
        return rng
    if _default_rng is None:
        _default_rng = SampleRNG()
    return _default_rng


def sample_rows(logits, top_k=None, top_p=None, min_p=None, temp=1.0, *, rng=None, uniforms=None):
    """logits (b, v), bf16 or fp32, unit inner stride and any row stride (``x[:, -1, :]`` needs no copy) -> next token ids int64 (b, 1), one launch.

    The meaning of ``sampling`` in fp32, with its gaps closed (include/mi355_vlm.h: mi355_sample_rows): the filter is ``min_p`` if set and non-zero, else
    ``top_p``, else ``top_k``, else none; ``top_p`` with ``min_p`` raises.  Top-k keeps the lower token index among equal values at the k-th place; top-p
    walks the tokens in descending probability, lower index first among equals, and keeps the shortest prefix whose mass exceeds ``top_p``, after dropping
    everything below the k-th largest value when ``top_k`` is given; min-p never drops the top ``top_k or 1`` tokens.  The draw returns the first kept
    token, in token-index order, whose running kept mass exceeds ``u`` times the kept mass.  ``u`` in [0, 1) per row comes from ``uniforms`` (fp32 (b,) on the
    device) or from ``rng`` (a ``SampleRNG``; None: one module-level stream seeded from ``torch.initial_seed()``), whose offset advances by one per call.
    ``temp == 0`` is greedy decoding (``argmax_rows``)."""
    B, V = KS.check_logits(logits)
    if temp == 0.0:
        if top_p is not None and min_p is not None:
            raise ValueError("sampling: cannot use top_p and min_p together")
        KS.L.require_gpu(logits)
        return ops_decode.argmax_rows(logits if logits.stride(-1) == 1 else logits.contiguous()).unsqueeze(-1)
    mode, k, p, mp = KS.resolve_mode(V, top_k, top_p, min_p, temp)
    if uniforms is not None:
        return KS.sample_rows(logits, mode, k, p, mp, temp, uniforms=uniforms)
    KS.L.require_gpu(logits)
    rng = _rng_or_default(rng)
    return KS.sample_rows(logits, mode, k, p, mp, temp, seed=rng.seed, offset=rng.advance())


def generate_batched_rollouts(input_tensor, model, max_gen, context_length, top_k=None, top_p=None, min_p=None, temp=0.0, eos_ids=50256, pad_id=50256,
                              device=torch.device("cuda"), last_real=None, *, attention_mask, rng=None, uniforms=None, sync_every=1):
    """``generate_batched_loop_kv_cache`` (RIGHT-padded prompts) on the sampling kernels: the rollouts of an RL step.

    The responses int64 (b, P + max_gen) and the key mask uint8 of the same shape are allocated once; the full-width mask goes to the cached forward as it
    is (no ``torch.cat`` per token).  Per generated token, outside the model's own step: ONE launch that samples every row (``sample_rows``; ``temp == 0``:
    top-k 1 of the same kernel, the first index of the row maximum) and does the loop's bookkeeping -- finished rows emit ``pad_id``, the token goes to its
    response column and to the next step's input, ``finished |= token in eos_ids``, the key-mask column is ``!finished`` after that update -- plus the
    position increment.  The host reads the count of unfinished rows (four bytes) every ``sync_every`` tokens: with ``sync_every=1`` the loop stops at the
    token that finishes the last row, as the reference does; with ``sync_every=n`` the result may carry up to ``n - 1`` trailing columns that are all
    ``pad_id``, which ``batched_responses_collator`` masks.  ``uniforms``: fp32 (max_gen, b) on the device, row i drives token i (tests, replays); else
    ``rng`` (a ``SampleRNG``).  ``P + max_gen > context_length`` raises before any launch."""
    if input_tensor.dim() != 2:
        raise ValueError(f"generate_batched_rollouts: input_tensor must be (b, prompt_len), got {tuple(input_tensor.shape)}")
    B, P = input_tensor.shape
    max_gen, sync_every = int(max_gen), int(sync_every)
    if max_gen < 1 or sync_every < 1:
        raise ValueError(f"generate_batched_rollouts: max_gen and sync_every must be positive, got {max_gen} and {sync_every}")
    if P + max_gen > context_length:
        raise ValueError(f"generate_batched_rollouts: prompt_len + max_gen = {P + max_gen} exceeds the context length {context_length}")
    if tuple(attention_mask.shape) != (B, P):
        raise ValueError(f"generate_batched_rollouts: attention_mask must be ({B}, {P}), got {tuple(attention_mask.shape)}")
    if top_p is not None and min_p is not None:
        raise ValueError("sampling: cannot use top_p and min_p together")
    if temp < 0.0:
        raise ValueError(f"sampling: the temperature must be positive (0: greedy decoding), got {temp}")
    if uniforms is not None and (uniforms.dtype != torch.float32 or tuple(uniforms.shape) != (max_gen, B)):
        raise ValueError(f"generate_batched_rollouts: uniforms must be fp32 ({max_gen}, {B}), got {uniforms.dtype} {tuple(uniforms.shape)}")
    KS.eos_array(eos_ids)
    vocab = getattr(getattr(getattr(model, "out_head", None), "weight", None), "shape", (None,))[0]
    if vocab is not None:
        KS.resolve_mode(vocab, top_k, top_p, min_p, temp if temp != 0.0 else 1.0)
    if torch.device(device).type != "cuda" or (uniforms is not None and not uniforms.is_cuda):
        raise RuntimeError("generate_batched_rollouts runs only on an MI355X (HIP) device.  There is no CPU fallback for this path.")
    input_tensor = input_tensor.to(device)
    attention_mask = attention_mask.bool().to(device)
    if last_real is not None:
        last_real = last_real.to(device)
        next_pos = last_real.unsqueeze(-1) + 1
    else:
        next_pos = attention_mask.sum(dim=-1, keepdim=True)
        last_real = next_pos.squeeze(-1) - 1
    greedy = temp == 0.0
    if greedy:  # the first index of the row maximum, what argmax_rows gives
        top_k, top_p, min_p, temp = 1, None, None, 1.0
    elif uniforms is None:
        rng = _rng_or_default(rng)
    kv_cache = KVCache(num_layers=len(model.trf_blocks), prompt_len=P, context_len=context_length)
    done = 0
    with torch.inference_mode():
        state = KS.RolloutState(input_tensor, attention_mask, max_gen, eos_ids, pad_id)
        next_pos = next_pos.clone()
        logits = model(input_tensor, attn_mask=attention_mask, kv_cache=kv_cache)
        logits = logits[torch.arange(B, device=device), last_real, :]
        mode, k, p, mp = KS.resolve_mode(logits.shape[-1], top_k, top_p, min_p, temp)
        for i in range(max_gen):
            if uniforms is not None:
                KS.sample_rows(logits, mode, k, p, mp, temp, uniforms=uniforms[i], state=state, step=i)
            elif greedy:
                KS.sample_rows(logits, mode, k, p, mp, temp, seed=0, offset=0, state=state, step=i)
            else:
                KS.sample_rows(logits, mode, k, p, mp, temp, seed=rng.seed, offset=rng.advance(), state=state, step=i)
            done = i + 1
            if done == max_gen:
                break
            if done % sync_every == 0:
                KS.COUNTERS["host_reads"] += 1
                if state.live[i].item() == 0:
                    break
            logits = model(state.next_token, attn_mask=state.key_mask, kv_cache=kv_cache, position_ids=next_pos).squeeze(1)
            next_pos += 1
    return state.responses[:, : P + done].clone()
