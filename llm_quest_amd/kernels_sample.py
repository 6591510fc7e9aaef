"""Tensor-level launchers of the rollout kernels (csrc/sampling.hip): the row sampler with the rollout's per-token bookkeeping folded in, and the
response masks of ``batched_responses_collator``.

Every launcher checks its arguments on the host first (so a refusal reads the same with or without a GPU), then that the operands live on the device --
there is no CPU fallback -- and enqueues on torch's current stream.  ``COUNTERS`` counts what this module enqueued (``launches``) and what the rollout loop
read back from the device (``host_reads``); tests and tools/bench_rollout.py read it.
"""

import ctypes

import torch

from . import _lib as L

BF16, F32 = torch.bfloat16, torch.float32
NONE, TOP_K, TOP_P, MIN_P = 0, 1, 2, 3
MAX_V = 1 << 20
MAX_EOS = 8
COUNTERS = {"launches": 0, "host_reads": 0}


def resolve_mode(V, top_k=None, top_p=None, min_p=None, temp=1.0):
    """(mode, top_k, top_p, min_p) as the kernel takes them, by the reference's truthiness chain (generate.py:501-509): ``min_p`` if set and non-zero, else
    ``top_p``, else ``top_k``, else no filter; ``top_k`` rides along with ``top_p`` (the cut-off value) and ``min_p`` (the tokens always kept).  Host only."""
    if top_p is not None and min_p is not None:
        raise ValueError("sampling: cannot use top_p and min_p together")
    if not temp > 0.0 or temp != temp or temp == float("inf"):
        raise ValueError(f"sampling: the temperature must be positive and finite, got {temp} (0 is greedy decoding: argmax_rows)")
    k = int(top_k) if top_k else 0
    if k < 0 or k > V:
        raise ValueError(f"sampling: top_k must lie in 1..vocab_size ({V}), got {top_k}")
    if min_p:
        if not 0.0 < min_p <= 1.0:
            raise ValueError(f"sampling: min_p must lie in (0, 1], got {min_p}")
        return MIN_P, k, 0.0, float(min_p)
    if top_p:
        if not top_p > 0.0:
            raise ValueError(f"sampling: top_p must be positive, got {top_p}")
        return TOP_P, k, float(top_p), 0.0
    if k:
        return TOP_K, k, 0.0, 0.0
    return NONE, 0, 0.0, 0.0


def check_logits(logits):
    """(B, V) of a logits block the sampler can address in place: bf16 / fp32 [B, V], unit inner stride, any row stride >= V (``x[:, -1, :]`` is fine)."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2:
        raise ValueError(f"sampling: logits must be 2-D (b, vocab_size), got {tuple(getattr(logits, 'shape', ()))}")
    if logits.dtype not in (BF16, F32):
        raise TypeError(f"sampling: logits must be bf16 or fp32, got {logits.dtype}")
    B, V = logits.shape
    if B < 1 or B > 65535 or V < 1 or V > MAX_V:
        raise ValueError(f"sampling: 1 <= b <= 65535 rows of 1 <= vocab_size <= {MAX_V}, got {tuple(logits.shape)}")
    return B, V


def eos_array(eos_ids):
    """The EOS ids as the host array the entry points take: (ctypes array or None, n)."""
    ids = [] if eos_ids is None else ([int(e) for e in eos_ids] if isinstance(eos_ids, (list, tuple)) else [int(eos_ids)])
    if len(ids) > MAX_EOS:
        raise ValueError(f"sampling: at most {MAX_EOS} EOS ids, got {len(ids)}")
    return ((ctypes.c_int64 * len(ids))(*ids) if ids else None), len(ids)


class RolloutState:
    """The device buffers of one batched rollout, allocated once: ``responses`` int64 [B, P + max_gen] (the prompt copied in), ``key_mask`` uint8 of the same
    shape (the prompt's attention mask copied in, the rest 0), ``finished`` uint8 [B], ``next_token`` int64 [B, 1] and ``live`` int32 [max_gen] -- ``live[i]``
    receives the number of rows still unfinished after token i, the one small read the loop takes when a sync is due."""

    def __init__(self, input_tensor, attention_mask, max_gen, eos_ids, pad_id):
        B, P = input_tensor.shape
        dev = input_tensor.device
        self.P, self.max_gen = P, max_gen
        self.responses = torch.empty((B, P + max_gen), dtype=torch.int64, device=dev)
        self.responses[:, :P] = input_tensor
        self.key_mask = torch.zeros((B, P + max_gen), dtype=torch.uint8, device=dev)
        self.key_mask[:, :P] = attention_mask
        self.finished = torch.zeros((B,), dtype=torch.uint8, device=dev)
        self.next_token = torch.empty((B, 1), dtype=torch.int64, device=dev)
        self.live = torch.zeros((max(max_gen, 1),), dtype=torch.int32, device=dev)
        self.eos, self.n_eos = eos_array(eos_ids)
        self.pad_id = int(pad_id)


def sample_rows(logits, mode, top_k, top_p, min_p, temp, uniforms=None, seed=0, offset=0, state=None, step=0):
    """One token per row, int64 [B, 1]; ``mode`` etc. from ``resolve_mode``.  ``uniforms`` fp32 [B] on the device, or None: the kernel's Philox4x32-10 under
    ``(seed, offset)``.  With ``state`` (a ``RolloutState``) the launch also does the rollout's bookkeeping for generated token ``step`` and the result
    is ``state.next_token``."""
    B, V = check_logits(logits)
    if logits.stride(1) != 1 or logits.stride(0) < V:
        logits = logits.contiguous()
    if uniforms is not None and (uniforms.dtype != F32 or tuple(uniforms.shape) != (B,)):
        raise ValueError(f"sampling: uniforms must be fp32 [{B}], got {uniforms.dtype} {tuple(uniforms.shape)}")
    if state is not None and not 0 <= step < state.max_gen:
        raise ValueError(f"sampling: step {step} outside the rollout's {state.max_gen} tokens")
    if state is None:
        L.require_gpu(logits, uniforms)
        out = torch.empty((B, 1), dtype=torch.int64, device=logits.device)
        book = (None, None, 0, 0, None, 0, None, 0, 0, None)
    else:
        L.require_gpu(logits, uniforms, state.responses, state.key_mask, state.finished, state.next_token, state.live)
        if state.responses.shape[0] != B:
            raise ValueError(f"sampling: the rollout holds {state.responses.shape[0]} rows, the logits {B}")
        out = state.next_token
        book = (L.ptr(state.finished), state.eos, state.n_eos, state.pad_id, L.ptr(state.responses), state.responses.stride(0), L.ptr(state.key_mask),
                state.key_mask.stride(0), state.P + step, state.live.data_ptr() + 4 * step)
    if uniforms is not None and not uniforms.is_contiguous():
        uniforms = uniforms.contiguous()
    L.call("mi355_sample_rows", B, V, L.ptr(logits), L.dt_code(logits.dtype), logits.stride(0), mode, top_k, top_p, min_p, float(temp), L.ptr(uniforms),
           int(seed) & (2**64 - 1), int(offset) & (2**64 - 1), L.ptr(out), *book)
    COUNTERS["launches"] += 1
    return out


def response_masks(responses, prompt_masks, eos_ids, pad_token_id):
    """(attn_masks, reward_masks), bool [B, S], of ``batched_responses_collator`` (include/mi355_vlm.h: mi355_response_masks)."""
    if responses.dim() != 2 or responses.dtype != torch.int64:
        raise ValueError(f"response masks: responses must be int64 (b, s), got {responses.dtype} {tuple(responses.shape)}")
    B, S = responses.shape
    if prompt_masks.dim() != 2 or prompt_masks.shape[0] != B or prompt_masks.shape[1] > S:
        raise ValueError(f"response masks: shapes disagree: prompt_masks must be ({B}, <= {S}), got {tuple(prompt_masks.shape)}")
    if prompt_masks.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"response masks: prompt_masks must be bool or uint8, got {prompt_masks.dtype}")
    if B < 1 or S < 1:
        raise ValueError(f"response masks: empty responses {tuple(responses.shape)}")
    eos, n_eos = eos_array(eos_ids)
    P = prompt_masks.shape[1]
    L.require_gpu(responses, prompt_masks)
    if responses.stride(1) != 1:
        responses = responses.contiguous()
    pm = prompt_masks.contiguous().view(torch.uint8)
    attn = torch.empty((B, S), dtype=torch.uint8, device=responses.device)
    reward = torch.empty((B, S), dtype=torch.uint8, device=responses.device)
    L.call("mi355_response_masks", B, S, P, L.ptr(responses), responses.stride(0), L.ptr(pm), max(pm.stride(0), P), eos, n_eos, int(pad_token_id), L.ptr(attn),
           L.ptr(reward))
    COUNTERS["launches"] += 1
    return attn.view(torch.bool), reward.view(torch.bool)
