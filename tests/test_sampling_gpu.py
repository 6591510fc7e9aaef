"""The rollout kernels (csrc/sampling.hip) against their fp64 restatement (tests/sampling_oracle.py) and the reference transcript of the fixture
(tools/gen_golden_rollout.py).  Every comparison is on integers and exact: the margins that make that legitimate -- ``top_p`` and ``min_p * p_max`` at least
1e-4 (relative) from a decision, every uniform at the midpoint of the CDF interval of a token with 1e-3 of the mass -- are asserted first."""

import json
import os

import numpy as np
import pytest
import torch
from safetensors.torch import load_file

import sampling_oracle as SO

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BF16, F32 = torch.bfloat16, torch.float32
BIG_V = 151936
GRID = [(V, B) for V in (1, 7, 64, 255, 256, 257, 1000, 4099) for B in (1, 3, 64)] + [(BIG_V, 2)]


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from llm_quest_amd import _lib, generate, kernels_sample

    _lib.load()
    return kernels_sample, generate, torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "rollout_signatures.json")) as f:
        meta = json.load(f)
    return load_file(os.path.join(GOLDEN, "rollout_tiny.safetensors")), meta


def base_for(t, V):
    """The fixture's rows where it has them (V <= 4 099), else rows made here (their margins are asserted like the fixture's)."""
    return t[f"base.{V}"] if f"base.{V}" in t else SO.base_rows(V, 0)


def layouts(x, dev):
    """The same rows contiguous, as the last position of a (B, 2, V) tensor, and inside rows of V + 3 elements starting at element 1: an odd pitch and a
    row start that breaks 16-byte alignment."""
    B, V = x.shape
    xd = x.to(dev)
    mid = torch.zeros(B, 2, V, dtype=x.dtype, device=dev)
    mid[:, -1, :] = xd
    odd = torch.zeros(B, V + 3, dtype=x.dtype, device=dev)
    odd[:, 1 : V + 1] = xd
    return {"contiguous": xd, "x[:, -1, :]": mid[:, -1, :], "odd pitch": odd[:, 1 : V + 1]}


def scripted(x, temp, kw, pick, margin):
    """(uniforms fp32 [B], the oracle's tokens) with the margin conditions asserted."""
    info = SO.sample_oracle(x, temp=temp, **kw)
    assert info["margin_p"].min() >= margin and info["margin_min_p"].min() >= margin, "the inputs sit on a decision boundary"
    u, tok = SO.midpoint_uniforms(info, pick=pick)
    drawn = SO.draw(info, u)
    assert np.array_equal(drawn["token"], tok) and drawn["margin_u"].min() >= 4e-4
    return u, tok


@pytest.mark.parametrize("V,B", GRID)
def test_sampler_against_the_oracle(env, fixture, V, B):
    """Every configuration (top-k 1, 2, 20, 64, V; top-p 0.5 and 0.9 alone and with top-k 20; min-p 0.1 alone and with top-k 5; no filter) at every
    temperature (1e-3, 0.7, 1, 1.5), in bf16 and fp32, in three memory layouts; where B V exceeds 32 000 (the restatement's own time) each configuration
    runs at one of the four temperatures in turn.
    The chosen tokens equal the oracle's for every row."""
    KS, G, dev = env
    t, meta = fixture
    base = base_for(t, V)
    wrong, runs = [], 0
    for mi, (name, kw) in enumerate(SO.modes_for(V)):
        for temp in (SO.TEMPS if V * B <= 32000 else (SO.TEMPS[mi % 4],)):
            for dtype in (BF16, F32):
                x = SO.spread_rows(SO.logits_from_base(base, temp, dtype, 10.0 if V == BIG_V else 3.0), B)
                u, tok = scripted(x, temp, kw, mi, meta["margin"])
                ud = torch.from_numpy(u).to(dev)
                for layout, xd in layouts(x, dev).items():
                    got = G.sample_rows(xd, temp=temp, uniforms=ud, **kw)
                    assert got.dtype == torch.int64 and tuple(got.shape) == (B, 1)
                    runs += 1
                    if not np.array_equal(got.cpu().numpy()[:, 0], tok):
                        wrong.append(f"{name} temp {temp} {dtype} {layout}: {got.cpu().numpy()[:, 0].tolist()} against {tok.tolist()}")
    assert not wrong, f"{len(wrong)} of {runs} runs differ:\n" + "\n".join(wrong[:10])


def test_special_rows(env, fixture):
    """All-equal logits, one dominant logit, rows with -inf entries, ties straddling the boundary, u = 0 and u = 1 - 2^-24."""
    KS, G, dev = env
    t, meta = fixture
    lo, hi = np.float32(0.0), np.float32(1 - 2.0**-24)

    def run(x, u, edge=None, **kw):
        u = np.broadcast_to(np.asarray(u, dtype=np.float32), (x.shape[0],)).copy()
        want = SO.sample_oracle(x, u=u, **kw)
        assert want["margin_p"].min() >= meta["margin"] and want["margin_min_p"].min() >= meta["margin"], "the inputs sit on a decision boundary"
        for b in range(x.shape[0]):  # the draw must not hang on rounding: away from every CDF step, or -- at the two ends -- on a token with real mass
            live = np.nonzero(want["kept"][b] & (want["p"][b] > 0))[0]
            if edge == "lo":
                assert want["token"][b] == live[0] and want["probs"][b, live[0]] >= 1e-30
            elif edge == "hi":
                assert want["token"][b] == live[-1] and want["probs"][b, live[-1]] >= 1e-3
            else:
                assert want["margin_u"][b] >= 1e-5
        got = G.sample_rows(x.to(dev), uniforms=torch.from_numpy(u).to(dev), **kw).cpu().numpy()[:, 0]
        assert np.array_equal(got, want["token"]), (kw, u.tolist(), got.tolist(), want["token"].tolist())
        assert all(want["kept"][b, got[b]] and want["p"][b, got[b]] > 0 for b in range(x.shape[0])), "a dropped or -inf token came back"
        return got, want

    small = [{"top_k": 5}, {"top_p": 0.5}, {"top_p": 0.9, "top_k": 5}, {"min_p": 0.1}, {"min_p": 0.1, "top_k": 5}]
    for dtype in (BF16, F32):
        flat = torch.full((2, 701), 0.25, dtype=dtype)  # all equal: every tie rule at once, across two wave tiles
        for kw in small + [{}]:
            got, want = run(flat, np.float32(0.5003), **kw)
            kept = np.nonzero(want["kept"][0])[0]
            assert run(flat, lo, "lo", **kw)[0][0] == kept[0] and run(flat, hi, "hi", **kw)[0][0] == kept[-1]
        peak = torch.zeros(2, 1000, dtype=dtype)  # one dominant logit
        peak[0, 123], peak[1, 999] = 40.0, 40.0
        for kw in small + [{}]:
            got, _ = run(peak, [0.3, 0.99], **kw)
            assert got.tolist() == [123, 999]
        holes = SO.logits_from_base(base_for(t, 257), 1.0, dtype).clone()  # -inf entries, among them the first and the last token
        holes[:, ::3] = -float("inf")
        holes[:, -1] = -float("inf")
        for kw in small:
            run(holes, lo, "lo", **kw), run(holes, hi, "hi", **kw), run(holes, np.float32(0.37), **kw)
        for kw in ({}, {"top_k": 200}, {"top_k": 257}):  # more places than finite logits: the -inf tokens still never come back
            run(holes, lo, "lo", **kw), run(holes, np.float32(0.37), **kw), run(holes, np.float32(0.93), **kw)
    for name, kw in meta["ties"].items():  # the fixture's tie rows: the lower index stays (top-k, top-p, min-p); all ties stay candidates (top-p with top-k)
        for dtype in (BF16, F32):
            x = t[f"tie.{name}.x"].to(dtype).unsqueeze(0)
            want = SO.sample_oracle(x, **kw)
            kept = np.nonzero(want["kept"][0])[0]
            assert run(x, lo, "lo", **kw)[0][0] == kept[0] and run(x, hi, "hi", **kw)[0][0] == kept[-1]
            for j in kept:  # every kept token is reachable at the midpoint of its interval, no other is
                u = np.float32(want["cdf"][0, j] - 0.5 * want["probs"][0, j])
                assert run(x, u, **kw)[0][0] == j


def test_generator_mode(env, fixture):
    """With ``SampleRNG`` the tokens are the oracle's under the Python Philox's uniforms; a row's token does not depend on the batch around it; every call
    advances the offset by one."""
    KS, G, dev = env
    t, _ = fixture
    x = SO.spread_rows(SO.logits_from_base(base_for(t, 1000), 1.0, BF16), 64)
    for seed, offset in ((0, 0), (1234, 7), ((1 << 40) + 99, 3), ((1 << 63) + 5, (1 << 32) + 1)):
        rng = G.SampleRNG(seed)
        rng.offset = offset
        got = G.sample_rows(x.to(dev), top_k=20, temp=1.0, rng=rng).cpu().numpy()[:, 0]
        u = SO.philox_uniforms(seed, offset, 64)
        want = SO.sample_oracle(x, top_k=20, temp=1.0, u=u)
        sure = want["margin_u"] >= 1e-5  # a uniform within fp32 rounding of a CDF step decides nothing
        assert sure.sum() >= 60 and np.array_equal(got[sure], want["token"][sure])
        assert rng.offset == offset + 1
        rng.offset = offset
        small = G.sample_rows(x[:5].to(dev), top_k=20, temp=1.0, rng=rng).cpu().numpy()[:, 0]
        assert np.array_equal(small, got[:5]), "a row's draw depends on (seed, offset, row) alone"
        again = G.sample_rows(x.to(dev), top_k=20, temp=1.0, rng=rng).cpu().numpy()[:, 0]
        assert rng.offset == offset + 2 and not np.array_equal(again, got)
        want2 = SO.sample_oracle(x, top_k=20, temp=1.0, u=SO.philox_uniforms(seed, offset + 1, 64))
        sure = want2["margin_u"] >= 1e-5
        assert np.array_equal(again[sure], want2["token"][sure])


def test_greedy_equivalence(env):
    """``top_k=1, temp=1.0`` is ``argmax_rows``: the first index of the row maximum, ties included; ``temp=0`` goes there directly."""
    KS, G, dev = env
    from llm_quest_amd import ops_decode

    g = torch.Generator().manual_seed(3)
    x = (torch.randn(7, 5000, generator=g) * 2).to(BF16)
    x[0, 17] = x[0, 4100] = x[0].max() + 1  # a tie for the maximum
    x[3, :] = 0.5
    xd = x.to(dev)
    want = ops_decode.argmax_rows(xd).cpu()
    assert want[0] == 17 and want[3] == 0
    for u in (0.0, 0.999):
        got = G.sample_rows(xd, top_k=1, temp=1.0, uniforms=torch.full((7,), u, device=dev))
        assert torch.equal(got.cpu()[:, 0], want)
    assert torch.equal(G.sample_rows(xd, temp=0.0).cpu()[:, 0], want)
    assert torch.equal(G.sample_rows(xd, top_k=1, temp=1.0, rng=G.SampleRNG(5)).cpu()[:, 0], want)


def test_response_masks_against_the_fixture(env, fixture):
    """A prompt that contains the pad id, a response with no stop token, a stop token in the first response column, P = 1."""
    KS, G, dev = env
    from llm_quest_amd.alignment.rlhf_grpo.grpo_engine import batched_responses_collator

    t, meta = fixture
    for k, m in meta["responses"].items():
        resp, pm = t[f"resp.{k}.responses"].to(dev), t[f"resp.{k}.prompt_masks"].bool().to(dev)
        out = batched_responses_collator(resp, pm, device=dev, eos_ids=m["eos_ids"], pad_token_id=m["pad_token_id"])
        assert out["attn_masks"].dtype == torch.bool and out["reward_masks"].dtype == torch.bool
        assert torch.equal(out["attn_masks"].cpu(), t[f"resp.{k}.attn_masks"].bool()), k
        assert torch.equal(out["reward_masks"].cpu(), t[f"resp.{k}.reward_masks"].bool()), k
        assert torch.equal(out["padded_responses"].cpu(), t[f"resp.{k}.padded_responses"])
    wide = torch.full((3, 200), 11, dtype=torch.long)  # rows longer than one wave's stride; a view with a pitch of its own
    wide[0, 150], wide[0, 199], wide[1, 64], wide[1, 65] = 7, 3, 3, 7
    wide[2, 100], wide[2, 101], wide[2, 170] = 3, 3, 7
    pm = torch.ones(3, 70, dtype=torch.bool)
    pm[1, 60:] = False
    attn, reward = SO.response_masks(wide[:, :180].numpy(), pm.numpy(), [7], 3)
    out = batched_responses_collator(wide.to(dev)[:, :180], pm.to(dev), device=dev, eos_ids=[7], pad_token_id=3)
    assert np.array_equal(out["attn_masks"].cpu().numpy(), attn) and np.array_equal(out["reward_masks"].cpu().numpy(), reward)


class CannedModel:
    """The fixture's stub: returns the canned logits and records what each call was given."""

    def __init__(self, canned, last_real, P, dev):
        self.trf_blocks = [None]
        self.canned, self.last_real, self.P, self.dev = canned.to(dev), last_real.to(dev), P, dev
        self.calls = []

    def __call__(self, x, attn_mask=None, kv_cache=None, position_ids=None):
        i = len(self.calls)
        self.calls.append({"x": x.clone(), "attn_mask": attn_mask.clone(), "position_ids": None if position_ids is None else position_ids.clone()})
        B, V = self.canned.shape[1:]
        if i == 0:
            out = torch.zeros(B, self.P, V, device=self.dev)
            out[torch.arange(B, device=self.dev), self.last_real] = self.canned[0]
            return out
        return self.canned[i].unsqueeze(1)


@pytest.mark.parametrize("name", ["ragged", "early"])
def test_rollout_reproduces_the_reference_transcript(env, fixture, name):
    """``generate_batched_rollouts`` on the canned-logits stub under the scripted uniforms: the reference's returned tensor, its ``position_ids`` per call, a
    key mask equal to its ``attn_mask`` on the columns filled so far; per generated token one sampler launch, and one 4-byte read only when a sync is due.
    With ``sync_every=4`` the result differs by trailing all-pad columns only."""
    KS, G, dev = env
    t, meta = fixture
    spec = meta["scenarios"][name]
    P, pre = spec["P"], f"roll.{name}."
    want = t[pre + "out"]

    def run(sync_every):
        model = CannedModel(t[pre + "canned"], t[pre + "last_real"], P, dev)
        before = dict(KS.COUNTERS)
        out = G.generate_batched_rollouts(t[pre + "prompts"], model, spec["max_gen"], 64, eos_ids=spec["eos_ids"], pad_id=spec["pad_id"], device=dev,
                                          last_real=t[pre + "last_real"], attention_mask=t[pre + "mask"].bool(), uniforms=t[pre + "uniforms"].to(dev),
                                          sync_every=sync_every, **meta["roll_sampling"])
        return out.cpu(), model, {k: KS.COUNTERS[k] - before[k] for k in before}

    out, model, used = run(1)
    assert torch.equal(out, want) and not out.is_inference()
    assert len(model.calls) == meta["calls"][name]["model"]
    for i, c in enumerate(model.calls):
        ref_mask = t[f"{pre}call{i}.attn_mask"].bool()
        assert torch.equal(c["attn_mask"].cpu()[:, : ref_mask.shape[1]].bool(), ref_mask), f"call {i}: the key mask differs on the filled columns"
        if i:
            assert c["attn_mask"].dtype == torch.uint8 and c["attn_mask"].shape[1] == P + spec["max_gen"], "the full-width buffer goes to the model as it is"
            assert torch.equal(c["position_ids"].cpu(), t[f"{pre}call{i}.position_ids"]), f"call {i}: position_ids"
            assert torch.equal(c["x"].cpu(), want[:, P + i - 1 : P + i])
        else:
            assert c["position_ids"] is None
    tokens = want.shape[1] - P
    assert used["launches"] == tokens, "one sampler launch per generated token (the position increment is the only other launch outside the model)"
    assert used["host_reads"] == (tokens if tokens < spec["max_gen"] else tokens - 1)
    out4, model4, used4 = run(4)
    extra = out4.shape[1] - want.shape[1]
    assert 0 <= extra <= 3 and torch.equal(out4[:, : want.shape[1]], want) and bool((out4[:, want.shape[1]:] == spec["pad_id"]).all())
    assert used4["host_reads"] == (out4.shape[1] - P) // 4 - (1 if out4.shape[1] - P == spec["max_gen"] and spec["max_gen"] % 4 == 0 else 0)
    assert used4["launches"] == out4.shape[1] - P
    if name == "early":
        assert extra == 1 and want.shape[1] - P == 3, "all rows finish at token 2: sync_every=1 stops there, sync_every=4 one pad column later"


TINY = dict(vocab_size=1000, emb_dim=128, n_layers=2, n_heads=4, num_kv_groups=2, head_dim=128, hidden_dim=256, context_length=64, rope_base=1_000_000,
            dtype=BF16, tie_embeddings=True)


def test_rollout_on_a_tiny_qwen3(env):
    """B = 6 ragged prompts of 5..9 tokens, max_gen = 8: ``top_k=1, temp=1.0`` equals ``generate_batched_loop_kv_cache(temp=0.0)`` token for token, and a fixed
    ``rng`` seed reproduces the same sampled responses twice."""
    KS, G, dev = env
    from llm_quest_amd.alignment.rlhf_grpo.grpo_engine import rlhf_grpo_prompt_collator
    from llm_quest_amd.qwen.qwen3.qwen3_model import Qwen3Model

    torch.manual_seed(0)
    model = Qwen3Model(dict(TINY)).to(dev).eval()
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(10, 1000, (n,), generator=g).tolist() for n in (5, 9, 7, 6, 8, 9)]
    batch = rlhf_grpo_prompt_collator(prompts, pad_token_id=3, device=dev)
    common = dict(eos_ids=[7, 9], pad_id=3, device=dev, last_real=batch["last_real_pos"], attention_mask=batch["prompt_masks"])
    want = G.generate_batched_loop_kv_cache(batch["padded_prompts"], model, 8, 64, temp=0.0, **common)
    got = G.generate_batched_rollouts(batch["padded_prompts"], model, 8, 64, top_k=1, temp=1.0, **common)
    assert torch.equal(got, want)
    assert torch.equal(G.generate_batched_rollouts(batch["padded_prompts"], model, 8, 64, temp=0.0, **common), want)
    a = G.generate_batched_rollouts(batch["padded_prompts"], model, 8, 64, top_k=20, temp=1.0, rng=G.SampleRNG(11), **common)
    b = G.generate_batched_rollouts(batch["padded_prompts"], model, 8, 64, top_k=20, temp=1.0, rng=G.SampleRNG(11), **common)
    c = G.generate_batched_rollouts(batch["padded_prompts"], model, 8, 64, top_k=20, temp=1.0, rng=G.SampleRNG(12), **common)
    assert torch.equal(a, b) and a.shape == (6, 9 + 8) and not torch.equal(a, c)
    assert torch.equal(a[:, :9], batch["padded_prompts"]) and bool(((a[:, 9:] >= 0) & (a[:, 9:] < 1000)).all())
    with pytest.raises(ValueError, match="context length"):
        G.generate_batched_rollouts(batch["padded_prompts"], model, 56, 64, temp=1.0, **common)
