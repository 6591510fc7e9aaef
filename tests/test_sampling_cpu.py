"""CPU checks of the rollout sampler's restatement (tests/sampling_oracle.py) against the fixture that tools/gen_golden_rollout.py recorded from the
reference, of the fixture's own strength, and of the host-side refusals of ``sample_rows`` / ``generate_batched_rollouts``."""

import inspect
import json
import os

import numpy as np
import pytest
import torch
from safetensors.torch import load_file

import sampling_oracle as SO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "rollout_signatures.json")) as f:
        meta = json.load(f)
    return load_file(os.path.join(GOLDEN, "rollout_tiny.safetensors")), meta


def case_logits(t, meta, key):
    V, c = int(key.split(".")[0]), meta["cases"][key]
    return SO.logits_from_base(t[f"base.{V}"], c["temp"], DTYPES[c["dtype"]]), c


def test_philox_known_answers():
    """Philox4x32-10's published known-answer vectors (counter words, key words -> output words)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for counter, key, want in kat:
        assert SO.philox4x32_10(counter, key) == want
    u = SO.philox_uniform((1 << 40) + 5, (1 << 33) + 2, 3)
    assert 0.0 <= u < 1.0 and u == (SO.philox4x32_10((3, 0, 2, 2), (5, 1 << 8))[0] >> 8) * 2.0**-24


def test_oracle_matches_the_reference_on_every_fixture_case(fixture):
    """Kept sets equal the reference's (``probs > 0``) exactly; the renormalised probabilities agree with its fp32 values within 4 x the floor the generator
    measured (the reference's fp32 run against its fp64 run) per case."""
    t, meta = fixture
    assert len(meta["cases"]) >= 70
    for key in meta["cases"]:
        x, c = case_logits(t, meta, key)
        info = SO.sample_oracle(x, temp=c["temp"], **c["kwargs"])
        ref = t[f"probs.{key}"].double().numpy()
        assert np.array_equal(info["kept"], ref > 0), key
        assert [int(n) for n in info["kept"].sum(axis=1)] == c["kept"], key
        worst = np.abs(info["probs"] - ref).max()
        assert worst <= 4 * c["floor"] + 1e-12, f"{key}: {worst:.3e} against a floor of {c['floor']:.3e}"


def test_fixture_conditions(fixture):
    """A weak fixture cannot pass: the margins, the scripted uniforms, a strict subset and a boundary tie per mode."""
    t, meta = fixture
    strict = {"top_k": False, "top_p": False, "min_p": False}
    for key in meta["cases"]:
        x, c = case_logits(t, meta, key)
        kw = c["kwargs"]
        info = SO.sample_oracle(x, temp=c["temp"], **kw)
        assert info["margin_p"].min() >= meta["margin"] and info["margin_min_p"].min() >= meta["margin"], key
        assert not info["boundary_tie"].any(), key
        u, tok = SO.midpoint_uniforms(info)
        drawn = SO.sample_oracle(x, temp=c["temp"], u=u, **kw)
        assert np.array_equal(drawn["token"], tok), key
        for b in range(x.shape[0]):
            j = tok[b]
            assert info["probs"][b, j] >= 1e-3
            lo = info["cdf"][b, j] - info["probs"][b, j]
            assert abs(float(u[b]) - (lo + info["cdf"][b, j]) / 2) <= 1e-7, "the scripted uniform sits at the midpoint of its token's interval"
        mode = "min_p" if kw.get("min_p") else "top_p" if kw.get("top_p") else "top_k" if kw.get("top_k") else None
        if mode and (info["kept"].sum(axis=1) < x.shape[1]).all() and (info["kept"].sum(axis=1) > 0).all():
            strict[mode] = True
    assert all(strict.values()), strict
    assert {"top_k", "top_p", "top_p_top_k", "min_p"} <= set(meta["ties"])


def test_tie_cases_follow_the_oracles_definition(fixture):
    """Ties at the boundary are this project's definition (torch leaves them open): the lower token index stays for top-k, for top-p's walk and for min-p's
    always-kept tokens; every tie at the k-th value stays a candidate of top-p with top-k."""
    t, meta = fixture
    want = {"top_k": [5, 11, 50], "top_p_top_k": [5, 11, 29, 40, 50], "top_p": [9, 20, 33], "min_p": [8, 17]}
    for name, kw in meta["ties"].items():
        x = t[f"tie.{name}.x"]
        assert torch.equal(x.to(torch.bfloat16).float(), x), "bf16 holds the tie rows exactly"
        info = SO.sample_oracle(x, temp=1.0, **kw)
        assert sorted(np.nonzero(info["kept"][0])[0].tolist()) == want[name], name
        assert bool(info["boundary_tie"][0]) == (name != "top_p_top_k"), name
        assert info["margin_p"].min() >= meta["margin"] and info["margin_min_p"].min() >= meta["margin"]


def test_draw_edges_of_the_oracle():
    x = torch.tensor([[0.0, -float("inf"), 1.0, 1.0, -float("inf"), 0.5]])
    lo = SO.sample_oracle(x, u=np.float32(0.0))
    hi = SO.sample_oracle(x, u=np.float32(1 - 2.0**-24))
    assert lo["token"][0] == 0 and hi["token"][0] == 5
    k2 = SO.sample_oracle(x, top_k=2, u=np.float32(1 - 2.0**-24))
    assert sorted(np.nonzero(k2["kept"][0])[0].tolist()) == [2, 3] and k2["token"][0] == 3 and bool(k2["boundary_tie"][0]) is False
    assert SO.sample_oracle(x, top_k=1, u=np.float32(0.9))["token"][0] == 2, "top-k 1 is the first index of the maximum"


def test_response_masks_and_bookkeeping_of_the_oracle(fixture):
    """The oracle's response masks are bit-equal to the reference's on the fixture's batches; the per-token bookkeeping replays the reference transcript."""
    t, meta = fixture
    for k, m in meta["responses"].items():
        attn, reward = SO.response_masks(t[f"resp.{k}.responses"].numpy(), t[f"resp.{k}.prompt_masks"].numpy(), m["eos_ids"], m["pad_token_id"])
        assert np.array_equal(attn, t[f"resp.{k}.attn_masks"].numpy().astype(bool)), k
        assert np.array_equal(reward, t[f"resp.{k}.reward_masks"].numpy().astype(bool)), k
        assert torch.equal(t[f"resp.{k}.padded_responses"], t[f"resp.{k}.responses"])
    for name, spec in meta["scenarios"].items():
        canned, u = t[f"roll.{name}.canned"], t[f"roll.{name}.uniforms"].numpy()
        P, out = spec["P"], t[f"roll.{name}.out"].numpy()
        finished = np.zeros(spec["B"], dtype=bool)
        for i in range(out.shape[1] - P):
            info = SO.sample_oracle(canned[i], u=u[i], **meta["roll_sampling"])
            token, finished, col = SO.rollout_step(info["token"], finished, spec["eos_ids"], spec["pad_id"])
            assert np.array_equal(token, out[:, P + i]), (name, i)
            later = f"roll.{name}.call{i + 1}.attn_mask"
            if later in t:
                assert np.array_equal(col, t[later].numpy()[:, P + i].astype(bool))
        assert finished.all() == (name == "early")
        assert out.shape[1] - P == meta["calls"][name]["sampler"] and (name != "early" or out.shape[1] - P < spec["max_gen"])


def test_signatures(fixture):
    """This project's new names carry the parameter lists the generator recorded; the rollout function is the reference's batched loop plus the listed
    keyword extensions."""
    from llm_quest_amd import generate as G

    _, meta = fixture
    sig = lambda fn: [[n, None if p.default is inspect.Parameter.empty else repr(p.default)] for n, p in inspect.signature(fn).parameters.items()]
    ours = meta["signatures"]["ours"]
    assert sig(G.SampleRNG.__init__) == ours["SampleRNG"] and sig(G.sample_rows) == ours["sample_rows"]
    assert sig(G.generate_batched_rollouts) == ours["generate_batched_rollouts"]
    ref = meta["signatures"]["reference"]
    assert sig(G.generate_batched_rollouts) == ref["generate_batched_loop_kv_cache"] + [["rng", "None"], ["uniforms", "None"], ["sync_every", "1"]]
    assert sig(G.generate_batched_loop_kv_cache) == ref["generate_batched_loop_kv_cache"] and sig(G.sampling) == ref["sampling"]
    kinds = inspect.signature(G.sample_rows).parameters
    assert [n for n, p in kinds.items() if p.kind is inspect.Parameter.KEYWORD_ONLY] == ["rng", "uniforms"]
    assert [n for n in kinds][:5] == [r[0] for r in ref["sampling"]] and kinds["temp"].default == 1.0


def test_sample_rng_is_host_state():
    from llm_quest_amd.generate import SampleRNG

    torch.manual_seed(1234)
    r = SampleRNG()
    assert r.seed == 1234 and r.offset == 0 and r.advance() == 0 and r.advance() == 1 and r.offset == 2
    assert SampleRNG((1 << 64) + 7).seed == 7 and SampleRNG(1 << 40).seed == 1 << 40


def test_refusals_without_a_gpu():
    from llm_quest_amd import generate as G

    x = torch.zeros(2, 16, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.sample_rows(x, top_k=4, temp=1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.sample_rows(x, temp=0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.sample_rows(x, top_p=0.9, uniforms=torch.zeros(2))
    with pytest.raises(ValueError, match="temperature"):
        G.sample_rows(x, top_k=4, temp=-1.0)
    with pytest.raises(ValueError, match="top_k"):
        G.sample_rows(x, top_k=17, temp=1.0)
    with pytest.raises(ValueError, match="top_p and min_p"):
        G.sample_rows(x, top_p=0.9, min_p=0.1)
    with pytest.raises(ValueError, match="uniforms"):
        G.sample_rows(x, top_k=2, uniforms=torch.zeros(3))
    with pytest.raises(TypeError, match="bf16 or fp32"):
        G.sample_rows(x.to(torch.float16), top_k=2)
    with pytest.raises(ValueError, match="2-D"):
        G.sample_rows(x[0], top_k=2)

    class Stub:
        trf_blocks = [None]

    ids, mask = torch.zeros(2, 5, dtype=torch.long), torch.ones(2, 5, dtype=torch.bool)
    with pytest.raises(ValueError, match="context length"):
        G.generate_batched_rollouts(ids, Stub(), 60, 64, attention_mask=mask)
    with pytest.raises(ValueError, match="temperature"):
        G.generate_batched_rollouts(ids, Stub(), 4, 64, temp=-0.5, attention_mask=mask)
    with pytest.raises(ValueError, match="top_p and min_p"):
        G.generate_batched_rollouts(ids, Stub(), 4, 64, top_p=0.5, min_p=0.1, temp=1.0, attention_mask=mask)
    with pytest.raises(ValueError, match="EOS ids"):
        G.generate_batched_rollouts(ids, Stub(), 4, 64, eos_ids=list(range(9)), attention_mask=mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.generate_batched_rollouts(ids, Stub(), 4, 64, temp=1.0, top_k=3, device=torch.device("cpu"), attention_mask=mask)


def test_mode_chain_is_the_references_truthiness():
    from llm_quest_amd import kernels_sample as KS

    assert KS.resolve_mode(100, top_k=5, top_p=None, min_p=0.1) == (KS.MIN_P, 5, 0.0, 0.1)
    assert KS.resolve_mode(100, top_k=5, top_p=0.5) == (KS.TOP_P, 5, 0.5, 0.0)
    assert KS.resolve_mode(100, top_k=5, top_p=0.0) == (KS.TOP_K, 5, 0.0, 0.0)
    assert KS.resolve_mode(100, top_k=0, min_p=0.0) == (KS.NONE, 0, 0.0, 0.0) == KS.resolve_mode(100)
    assert KS.resolve_mode(100, top_k=100)[1] == 100
