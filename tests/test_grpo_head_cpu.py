"""CPU-side checks of the GRPO losses from hidden states: the fp32 restatement of the chunked flow (tests/grpo_head_oracle.py) against fp64 on the GPU
tests' planted logits, the chunk arithmetic of ``head_chunks``, every refusal of the launchers and the public names by message, the public names'
signatures and defaults, and the new entry points in header and binding table with their host-side validation (no launch)."""

import inspect
import os
import re

import pytest
import torch

import grpo_head_oracle as HO

BF16, F32, F64, I64 = torch.bfloat16, torch.float32, torch.float64, torch.int64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mi355_head_lse_chunk", "mi355_head_lse_finish", "mi355_head_dlogits_chunk")


def _engine():
    from llm_quest_amd.alignment.rlhf_grpo import grpo_engine

    return grpo_engine


@pytest.mark.parametrize("B,S,V,step", HO.ROW_CASES)
def test_chunked_restatement_against_fp64(B, S, V, step):
    """The fp32 chunked flow must be finite wherever a row has a finite entry (the row whose first chunk is all -inf included) and lie within one ulp of
    |lse| (half an ulp each for ``log l`` and the final addition) plus 1e-6 (the relative error of ``l``, a sum of at most V terms below 1, turned
    absolute by the logarithm) of the exact value; the fp64 chunked flow must be ``torch.logsumexp``."""
    c = HO.row_case(B, S, V, step)
    x = c["logits"][:, :-1]
    has_finite = torch.isfinite(x.float()).any(dim=-1)
    assert bool(has_finite.all()), "every planted row keeps a finite entry"
    for name in ("lse32", "lse64", "logp32", "logp64"):
        assert bool(torch.isfinite(c[name]).all()), f"{name} is not finite: {c['kinds']}"
    direct = torch.logsumexp(x.double(), dim=-1)
    assert float((c["lse64"] - direct).abs().max()) <= 1e-12
    err = (c["lse32"].double() - c["lse64"]).abs()
    bound = 2.0 ** -23 * c["lse64"].abs().clamp_min(1.0) + 1e-6
    direct32 = float((torch.logsumexp(x.float(), dim=-1).double() - c["lse64"]).abs().max())
    print(f"\n[{B, S, V, step}] kinds {sorted(set(c['kinds'].values()))}: worst lse error {float(err.max()):.3e} (torch.logsumexp in fp32: {direct32:.3e})")
    assert bool((err <= bound).all()), float(err.max())
    lab = c["ids_all"][:, :, 1:]
    want = x.double().unsqueeze(0).expand(lab.shape[0], -1, -1, -1).gather(-1, lab.unsqueeze(-1)).squeeze(-1) - direct
    assert float((c["logp64"] - want).abs().max()) <= 1e-12
    # a label outside [0, V) was in no chunk: NaN for its token only
    bad = c["ids_all"][0].clone()
    bad[B - 1, 1] = V
    lp, _ = HO.chunked_logprobs(c["logits"], bad, c["chunks"], F32)
    assert bool(torch.isnan(lp[B - 1, 0])) and int(torch.isnan(lp).sum()) == 1
    # the chunk gradient, concatenated, is the whole-row gradient of the existing restatement
    import grpo_oracle as GO

    if len(c["chunks"]) >= 2:
        g = torch.randn(B, S - 1, generator=torch.Generator().manual_seed(V))
        whole = GO.logprob_grad(c["logits"], c["ids_all"][0], g, F64)
        parts = torch.cat([HO.chunk_grad(c["logits"], c["ids_all"][0], g, c["lse64"], c0, c1, F64) for c0, c1 in c["chunks"]], dim=-1)
        assert GO.rel_l2(parts, whole) <= 1e-12


def test_special_rows_are_all_covered():
    seen = set()
    for case in HO.ROW_CASES:
        seen |= set(HO.row_case(*case)["kinds"].values())
    assert seen == set(HO.KINDS)


def test_head_chunks_arithmetic():
    from llm_quest_amd import kernels_grpo_head as KH

    assert KH.head_chunks(10, 24, 128) == [(0, 24)]  # V < chunk: clamped
    assert KH.head_chunks(10, 1003, 1024) == [(0, 1003)]
    assert KH.head_chunks(10, 24, 8) == [(0, 8), (8, 16), (16, 24)]  # V a multiple of the chunk
    assert KH.head_chunks(10, 9, 8) == [(0, 8), (8, 9)]  # a one-column tail
    assert KH.head_chunks(12, 1003, 128)[-1] == (896, 1003) and len(KH.head_chunks(12, 1003, 128)) == 8
    # the default rule: the largest multiple of 128 with rows * Vc * 2 B <= 128 MiB (the measured knee: DESIGN.md section 5), not below 1 024, clamped to V
    assert KH.CHUNK_BYTES == 128 << 20 and KH.CHUNK_MIN == 1024
    big = KH.head_chunks(4096, 151936)
    assert big[0] == (0, 16384) and big[-1] == (9 * 16384, 151936) and len(big) == 10
    assert 4096 * 16384 * 2 == KH.CHUNK_BYTES
    assert KH.head_chunks(16, 512) == [(0, 512)]
    assert KH.head_chunks(131072, 4096)[0] == (0, 1024)  # 128 MiB / (131 072 rows * 2 B) = 512 columns: the floor holds
    assert KH.head_chunks(5000, 151936)[0] == (0, 13312) and 13312 % 128 == 0 and 5000 * 13312 * 2 <= KH.CHUNK_BYTES < 5000 * (13312 + 128) * 2
    for c in (KH.head_chunks(4096, 151936), KH.head_chunks(12, 1003, 128)):
        assert c[0][0] == 0 and all(a[1] == b[0] for a, b in zip(c, c[1:])) and all(c0 % 8 == 0 for c0, _ in c)
    for bad in (0, -8, 12, 7, 8.5):
        with pytest.raises(ValueError, match="positive multiple of 8"):
            KH.head_chunks(10, 64, bad)
    with pytest.raises(ValueError, match="must be positive"):
        KH.head_chunks(0, 64)


def _sig(fn):
    return [[n, None if p.default is inspect.Parameter.empty else repr(p.default)] for n, p in inspect.signature(fn).parameters.items()]


def test_public_names_signatures_and_defaults():
    G = _engine()
    from llm_quest_amd.qwen.qwen3.qwen3_model import Qwen3Model

    assert _sig(G.log_probs_per_token_from_hidden) == [["hidden", None], ["out_head", None], ["inputs", None], ["vocab_chunk", "None"]]
    assert _sig(G.grpo_policy_loss_from_hidden) == [["hidden", None], ["out_head", None], ["inputs", None], ["old_logprobs", None], ["reference_logprobs", None],
                                                    ["advantages", None], ["loss_mask", None], ["num_samples", None], ["min_clip", None], ["max_clip", None],
                                                    ["beta", None], ["max_gen", "1"], ["variant", "'grpo'"], ["unbiased_kl_estimate", "False"],
                                                    ["off_policy_delta", "None"], ["vocab_chunk", "None"]]
    assert _sig(Qwen3Model.label_log_probs) == [["self", None], ["x", None], ["attn_mask", "None"], ["position_ids", "None"], ["vocab_chunk", "None"]]
    # everything behind ``inputs`` is grpo_policy_loss's own list, minus ``inplace`` (nothing is consumed here)
    assert _sig(G.grpo_policy_loss_from_hidden)[2:-1] == _sig(G.grpo_policy_loss)[1:-1]


class _Head(torch.nn.Module):
    def __init__(self, V=16, D=8, dtype=BF16):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.zeros(V, D, dtype=dtype))


def _operands(B=4, S=5, D=8, V=16):
    T = S - 1
    return dict(hidden=torch.zeros(B, S, D, dtype=BF16), out_head=_Head(V, D), inputs=torch.zeros(B, S, dtype=I64), old_logprobs=torch.zeros(B, T),
                reference_logprobs=torch.zeros(B, T), advantages=torch.ones(B), loss_mask=torch.ones(B, T, dtype=torch.bool), num_samples=2, min_clip=0.2,
                max_clip=0.2, beta=0.1)


def test_every_refusal_fires_by_message():
    G = _engine()
    from llm_quest_amd import kernels_grpo_head as KH

    ok = _operands()
    h, head, ids = ok["hidden"], ok["out_head"], ok["inputs"]
    w = head.weight.detach()
    T = ids.shape[1] - 1
    g = torch.zeros(4, T)
    public = ((lambda **kw: G.grpo_policy_loss_from_hidden(**dict(ok, **kw))),
              (lambda **kw: G.log_probs_per_token_from_hidden(kw.get("hidden", h), kw.get("out_head", head), kw.get("inputs", ids), kw.get("vocab_chunk"))))
    launchers = ((lambda **kw: KH.head_logprob_fwd(kw.get("hidden", h), kw.get("out_head", head).weight.detach(), kw.get("inputs", ids), kw.get("vocab_chunk"))),
                 (lambda **kw: KH.head_logprob_bwd(g, kw.get("hidden", h), kw.get("out_head", head).weight.detach(), g, kw.get("inputs", ids), kw.get("vocab_chunk"))))
    for fn in public + launchers:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()
        with pytest.raises(TypeError, match="hidden states must be bf16"):
            fn(hidden=h.float())
        with pytest.raises(ValueError, match=r"hidden states must be 3-D"):
            fn(hidden=h[0])
        with pytest.raises(TypeError, match="weight must be bf16"):
            fn(out_head=_Head(dtype=F32))
        with pytest.raises(TypeError, match=r"inputs must be int64 \[B, S\]"):
            fn(inputs=ids.int())
        with pytest.raises(TypeError, match=r"inputs must be int64 \[B, S\]"):
            fn(inputs=ids.flatten())
        with pytest.raises(ValueError, match="shapes disagree"):
            fn(inputs=ids[:, :-1])
        with pytest.raises(ValueError, match="shapes disagree"):
            fn(out_head=_Head(D=16))
        with pytest.raises(ValueError, match="emb_dim must be a multiple of 8"):
            fn(hidden=torch.zeros(4, 5, 12, dtype=BF16), out_head=_Head(D=12))
        with pytest.raises(ValueError, match="hidden states must be contiguous"):
            fn(hidden=torch.zeros(4, 5, 16, dtype=BF16)[:, :, :8])
        for bad in (12, 0, -8):
            with pytest.raises(ValueError, match="positive multiple of 8"):
                fn(vocab_chunk=bad)
    with pytest.raises(TypeError, match="out_head must be the model's output head"):
        G.log_probs_per_token_from_hidden(h, w, ids)
    with pytest.raises(TypeError, match="out_head must be the model's output head"):
        G.grpo_policy_loss_from_hidden(**dict(ok, out_head=torch.nn.Identity()))
    # the per-token operands of the loss: grpo_policy_loss's own refusals
    for key, bad in (("old_logprobs", torch.zeros(4, 5)), ("reference_logprobs", torch.zeros(3, 4)), ("advantages", torch.ones(5)),
                     ("loss_mask", torch.ones(4, 5, dtype=torch.bool)), ("old_logprobs", torch.zeros(4, 4, dtype=F64))):
        with pytest.raises(ValueError, match="shapes disagree"):
            G.grpo_policy_loss_from_hidden(**dict(ok, **{key: bad}))
    for variant in ("grpo", "sapo"):
        with pytest.raises(ValueError, match="not divisible by num_samples"):
            G.grpo_policy_loss_from_hidden(**dict(ok, num_samples=3, variant=variant))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.grpo_policy_loss_from_hidden(**dict(ok, num_samples=3, variant="gspo"))
    with pytest.raises(ValueError, match="Unknown loss type: ppo"):
        G.grpo_policy_loss_from_hidden(**dict(ok, variant="ppo"))
    with pytest.raises(ValueError, match="at least two positions"):
        G.grpo_policy_loss_from_hidden(**dict(ok, hidden=h[:, :1].contiguous(), inputs=ids[:, :1], old_logprobs=torch.zeros(4, 0),
                                              reference_logprobs=torch.zeros(4, 0), loss_mask=torch.zeros(4, 0)))
    # the backward's own operands
    with pytest.raises(ValueError, match="shapes disagree: g must be fp32"):
        KH.head_logprob_bwd(torch.zeros(4, 5), h, w, g, ids)
    with pytest.raises(ValueError, match="shapes disagree: lse must be fp32"):
        KH.head_logprob_bwd(g, h, w, g.double(), ids)
    with pytest.raises(ValueError, match="dw_out must be bf16 or fp32"):
        KH.head_logprob_bwd(g, h, w, g, ids, dw_out=torch.zeros(8, 16))
    with pytest.raises(ValueError, match="dw_out must be row-major"):
        KH.head_logprob_bwd(g, h, w, g, ids, dw_out=torch.zeros(8, 16).t())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KH.head_logprob_bwd(g, h, w, g, ids, dw_out=torch.zeros(16, 8))
    # the row launchers and the chunk GEMM
    chunk, state = torch.zeros(20, 16, dtype=BF16), torch.zeros(3, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KH.head_lse_chunk(chunk, 0, ids, state, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KH.head_lse_finish(state)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KH.head_dlogits_chunk(g, chunk, 0, 16, g, ids)
    with pytest.raises(TypeError, match="chunk must be bf16"):
        KH.head_lse_chunk(chunk.float(), 0, ids, state, True)
    with pytest.raises(ValueError, match="shapes disagree: chunk"):
        KH.head_lse_chunk(chunk[:19], 0, ids, state, True)
    with pytest.raises(ValueError, match="non-negative multiple of 8"):
        KH.head_lse_chunk(chunk, 4, ids, state, True)
    with pytest.raises(ValueError, match="non-negative multiple of 8"):
        KH.head_dlogits_chunk(g, chunk, -8, 16, g, ids)
    with pytest.raises(ValueError, match="16-byte rows"):
        KH.head_lse_chunk(torch.zeros(20, 20, dtype=BF16)[:, :16], 0, ids, state, True)  # a pitch of 20 elements
    with pytest.raises(ValueError, match="16-byte rows"):
        KH.head_lse_chunk(torch.zeros(20, 24, dtype=BF16)[:, 4:20], 0, ids, state, True)  # a pointer 8 bytes off
    with pytest.raises(ValueError, match="state must be contiguous fp32"):
        KH.head_lse_chunk(chunk, 0, ids, torch.zeros(3, 4, 5), True)
    with pytest.raises(ValueError, match="state must be contiguous fp32"):
        KH.head_lse_finish(torch.zeros(2, 4, 4))
    with pytest.raises(ValueError, match="does not lie inside the vocabulary"):
        KH.head_dlogits_chunk(g, chunk, 8, 16, g, ids)
    with pytest.raises(ValueError, match="shapes disagree: the output"):
        KH.head_dlogits_chunk(g, chunk, 0, 16, g, ids, out=torch.zeros(20, 8, dtype=BF16))
    with pytest.raises(ValueError, match="scratch must be contiguous bf16"):
        KH.head_chunk_logits(h.view(20, 8), w, 0, 12, torch.zeros(20, 12, dtype=BF16))


def test_qwen3_moe_refuses_label_log_probs_by_name():
    from llm_quest_amd.qwen.qwen3.qwen3_model import Qwen3MoEModel

    with pytest.raises(NotImplementedError, match="label_log_probs is built for the dense Qwen3Model"):
        Qwen3MoEModel.label_log_probs(None, None)


def test_entry_points_are_declared_bound_and_validate_on_the_host():
    from llm_quest_amd import _lib

    raw = open(os.path.join(ROOT, "include", "mi355_vlm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in ENTRY_POINTS:
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared in include/mi355_vlm.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name]), name
    head_part = raw[raw.index("GRPO losses from hidden states"):]
    for line in ("grpo_engine.py:397-425", ":413-425"):
        assert line in head_part, f"the header does not name the reference call site {line}"
    stubs = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert f"_lib.{name}.argtypes" in stubs, f"INTEGRATION.md has no stub of {name}"
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    buf = torch.zeros(64, dtype=F32)
    p = buf.data_ptr()  # a valid, 16-byte aligned host pointer: never dereferenced, every call below is refused first
    assert p % 16 == 0
    err = lambda: lib.mi355_last_error().decode()
    # null pointers and absurd sizes
    for B, S, Vc in ((1, 2, 8), (-1, 2, 8), (0, 2, 8), (1, 1, 8), (1, 2, 0), (1, 2, -8), (1 << 40, 1 << 40, 1 << 40)):
        assert lib.mi355_head_lse_chunk(B, S, Vc, 0, None, 8, None, None, None, None, 1, None) != 0 and "mi355_head_lse_chunk" in err()
        assert lib.mi355_head_dlogits_chunk(B, S, 8, Vc, 0, None, None, 8, None, None, None, 8, None) != 0 and "mi355_head_dlogits_chunk" in err()
    for n in (1, 0, -1, 1 << 60):
        assert lib.mi355_head_lse_finish(n, None, None, None, None, None, None) != 0 and "mi355_head_lse_finish" in err()
    assert lib.mi355_head_lse_finish(0, p, p, p, p, p, None) != 0 and "mi355_head_lse_finish" in err()
    assert lib.mi355_head_lse_chunk(1, 2, 8, 0, p, 8, p, p, p, None, 1, None) != 0 and "null pointer" in err()
    assert lib.mi355_head_dlogits_chunk(1, 2, 8, 8, 0, None, p, 8, p, p, p, 8, None) != 0 and "null pointer" in err()
    # the pitch, the pointer and the column offset: the vector path says what it needs
    lse = lambda Vc, c0, ptr, ld: lib.mi355_head_lse_chunk(1, 2, Vc, c0, ptr, ld, p, p, p, p, 1, None)
    assert lse(9, 0, p, 8) != 0 and "16-byte rows" in err()  # pitch < Vc
    assert lse(7, 0, p, 12) != 0 and "16-byte rows" in err()  # pitch no multiple of 8
    assert lse(8, 0, p + 2, 8) != 0 and "16-byte rows" in err()  # misaligned
    assert lse(8, 4, p, 8) != 0 and "16-byte rows" in err()  # c0 no multiple of 8
    assert lse(8, -8, p, 8) != 0 and "c0 in 0..2^31" in err()
    assert lib.mi355_head_lse_chunk(1 << 24, 1 << 24, 8, 0, p, 1 << 32, p, p, p, p, 1, None) != 0 and "64-bit element offset" in err()
    dl = lambda V, Vc, c0, src, ldc, dst, ldd: lib.mi355_head_dlogits_chunk(1, 2, V, Vc, c0, p, src, ldc, p, p, dst, ldd, None)
    assert dl(16, 9, 0, p, 8, p, 8) != 0 and "16-byte rows" in err()
    assert dl(16, 8, 0, p, 8, p, 12) != 0 and "16-byte rows" in err()
    assert dl(16, 8, 0, p, 8, p + 6, 8) != 0 and "16-byte rows" in err()
    assert dl(16, 8, -8, p, 8, p, 8) != 0 and "c0 in 0..2^31" in err()
    assert dl(16, 8, 16, p, 8, p, 8) != 0 and "inside the vocabulary" in err()
    assert dl(0, 8, 0, p, 8, p, 8) != 0 and "inside the vocabulary" in err()
    assert dl(16, 8, 0, p, 8, p, 16) != 0 and "in place" in err()
