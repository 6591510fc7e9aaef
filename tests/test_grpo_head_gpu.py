"""The GRPO losses from hidden states on the GPU: the row kernels of csrc/grpo_head.hip on planted logits (no GEMM involved), the composed path on random
hidden states and head weights, the loss against ``grpo_policy_loss`` on materialised logits, the memory the path is for, and a tiny Qwen3.

The yardsticks are those of tests/test_grpo_gpu.py: ``judge`` (at most 1.5 x as far from fp64 as the reference's bf16 flow), the element-wise distance of
the log-probs (at most 4 x the fp32 restatement's worst distance from fp64; the restatement here is the CHUNKED flow of tests/grpo_head_oracle.py), and
``_own_bound`` (at most 1.5 x the relative L2 distance of the kernels' own flow restated on the CPU).  The backward row kernel is held to the bits of
``mi355_label_logprob_bwd``.  The shapes are the smallest that cross an edge: a one-column vocabulary, a one-column tail chunk, a vocabulary that is no
multiple of 8, a chunk wider than the vocabulary, a chunk of 8 192 columns, more rows than one block walks at once.  Every figure is printed before it is
asserted (run with ``-s``)."""

import pytest
import torch

import grpo_head_oracle as HO
import grpo_oracle as GO
from test_deepseek_moe_gpu import judge
from test_grpo_gpu import GUARD, NAN, SC, TINY_QWEN, Pooled, _bits, _check, _guarded, _guards_intact, _own_bound, _place

pytestmark = pytest.mark.gpu

BF16, F32, F64, I64 = torch.bfloat16, torch.float32, torch.float64, torch.int64
COMPOSED_CASES = [(2, 5, 64, 24, 8), (2, 9, 128, 1000, 128), (3, 4, 72, 1003, 128), (4, 16, 128, 512, None)]


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from llm_quest_amd import _lib, kernels_grpo, kernels_grpo_head
    from llm_quest_amd.alignment.rlhf_grpo import grpo_engine

    _lib.load()
    return _lib, kernels_grpo, kernels_grpo_head, grpo_engine, torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fixture():
    return GO.load_fixture()


def _rows2d(buf, B, S, V):
    """The [B S, V] view of the logits ``_place`` put into ``buf`` (rows of pitch ceil8(V) behind the front guard)."""
    pitch = (V + 7) // 8 * 8
    return buf[GUARD:GUARD + B * S * pitch].view(B * S, pitch)[:, :V]


def _forward(KH, rows2d, chunks, ids, state):
    for i, (c0, c1) in enumerate(chunks):
        KH.head_lse_chunk(rows2d[:, c0:c1], c0, ids, state, first=i == 0)
    return KH.head_lse_finish(state)


def _elementwise(name, mine, own, exact, report):
    bound = 4.0 * float((own.double() - exact).abs().max())
    worst = float((mine.double() - exact).abs().max())
    print(f"  {name}: element-wise worst {worst:.3e}  bound 4 x fp32 restatement {bound:.3e}")
    if not worst <= bound:
        report.append(f"{name}: element-wise {worst:.3e} > {bound:.3e}")


# ----------------------------------------------------------------------------------------------------------------- row kernels on planted logits
@pytest.mark.parametrize("B,S,V,step", HO.ROW_CASES)
def test_row_kernels_forward(env, B, S, V, step):
    L, K, KH, G, dev = env
    c = HO.row_case(B, S, V, step)
    chunks, T = c["chunks"], S - 1
    buf, view, _ = _place(dev, c["logits"], False)
    rows2d = _rows2d(buf, B, S, V)
    before = buf.clone()
    runs = c["ids_all"].shape[0]
    ids_dev = c["ids_all"].to(dev)
    out = torch.empty((runs, 2, B, T), dtype=F32, device=dev)
    state_bufs = []
    for r in range(runs):
        sbuf, state = _guarded(dev, (3, B, T))  # NaN everywhere: what ``first`` must overwrite
        if r == 1 % runs:
            state.copy_(torch.tensor([1e30, 7.0, -3.0], device=dev).view(3, 1, 1).expand(3, B, T))  # a finite state left over from another case
        logp, lse = _forward(KH, rows2d, chunks, ids_dev[r], state)
        out[r, 0], out[r, 1] = logp, lse
        state_bufs.append(sbuf)
    again = torch.stack(_forward(KH, rows2d, chunks, ids_dev[0], torch.zeros((3, B, T), dtype=F32, device=dev)))
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf), _bits(before)), "the forward changed the logits or their surroundings"
    assert all(_guards_intact(s) for s in state_bufs), "a byte outside the state changed"
    assert not bool(torch.isnan(out).any()), "a sentinel survived in an output"
    assert torch.equal(_bits(again), _bits(out[0])), "two runs differ (or a state leaked through ``first``)"
    logp, lse = out[:, 0].cpu(), out[:, 1].cpu()
    report = []
    print(f"\n[head rows fwd {B, S, V, step}] {len(chunks)} chunks, {runs} label sets, kinds {sorted(set(c['kinds'].values()))}")
    judge("logp", logp, c["logp16"], c["logp64"], report)
    judge("lse", lse[0], c["lse16"], c["lse64"], report)
    _elementwise("logp", logp, c["logp32"], c["logp64"], report)
    _elementwise("lse", lse[0], c["lse32"], c["lse64"], report)
    for r in range(1, runs):
        assert torch.equal(_bits(lse[r]), _bits(lse[0])), "the labels changed a row's lse"
    # a label outside [0, V): NaN for its token only
    for bad_label in (-1, V):
        bad = ids_dev[0].clone()
        bad[B - 1, 1] = bad_label
        lp, ls = _forward(KH, rows2d, chunks, bad, torch.empty((3, B, T), dtype=F32, device=dev))
        nan = torch.isnan(lp)
        assert bool(nan[B - 1, 0]) and int(nan.sum()) == 1, "an out-of-range label must give NaN for its token only"
        assert torch.equal(_bits(lp)[~nan], _bits(out[0, 0])[~nan]) and torch.equal(_bits(ls), _bits(out[0, 1]))
    _check(report)


@pytest.mark.parametrize("B,S,V,step", [c for c in HO.ROW_CASES if len(HO.chunks_of(c[2], c[3])) >= 2])
def test_row_kernels_backward(env, B, S, V, step):
    """Bits equal to columns [c0, c1) of ``K.label_logprob_bwd`` fed the same (logits, lse, g, ids); in place equals out of place."""
    L, K, KH, G, dev = env
    c = HO.row_case(B, S, V, step)
    chunks, T = c["chunks"], S - 1
    g = torch.randn(B, T, generator=torch.Generator().manual_seed(7 + V)).to(dev)
    runs = c["ids_all"].shape[0]
    print(f"\n[head rows bwd {B, S, V, step}] {len(chunks)} chunks")
    for r in sorted({0, runs - 1}):
        ids = c["ids_all"][r].to(dev)
        buf, view, cov = _place(dev, c["logits"], False)
        rows2d = _rows2d(buf, B, S, V)
        before = buf.clone()
        _, lse = _forward(KH, rows2d, chunks, ids, torch.empty((3, B, T), dtype=F32, device=dev))
        want = K.label_logprob_bwd(g, view, lse, ids)  # the whole rows, out of place: existing code
        obuf, oview, ocov = _place(dev, torch.full((B, S, V), NAN, dtype=BF16), False)
        orows = _rows2d(obuf, B, S, V)
        for c0, c1 in chunks:
            obefore = obuf.clone()
            KH.head_dlogits_chunk(g, rows2d[:, c0:c1], c0, V, lse, ids, out=orows[:, c0:c1])
            inside = torch.zeros(obuf.shape, dtype=torch.bool, device=dev)
            _rows2d(inside, B, S, V)[:, c0:c1] = True
            assert torch.equal(_bits(obuf)[~inside], _bits(obefore)[~inside]), f"chunk {c0, c1}: a byte outside the chunk changed"
        torch.cuda.synchronize()
        assert torch.equal(_bits(buf), _bits(before)), "the out-of-place backward changed the logits"
        assert not bool(torch.isnan(oview).any()), "a sentinel survived in the output"
        same = torch.equal(_bits(oview), _bits(want))
        print(f"  set {r}: bits equal to label_logprob_bwd: {same}; differing elements {int((_bits(oview) != _bits(want)).sum())}")
        assert same, "the chunk gradients are not the bits of mi355_label_logprob_bwd"
        assert bool((_bits(oview[:, S - 1]) == 0).all()), "row S - 1 must be exact zeros"
        for c0, c1 in chunks:  # in place
            KH.head_dlogits_chunk(g, rows2d[:, c0:c1], c0, V, lse, ids)
        torch.cuda.synchronize()
        assert torch.equal(_bits(view), _bits(oview)), "in place differs from out of place"
        assert torch.equal(_bits(buf)[~cov], _bits(before)[~cov]), "the in-place backward changed a byte outside the logits"
    # a label outside [0, V): its row is exact zeros, as in mi355_label_logprob_bwd
    bad = c["ids_all"][0].clone()
    bad[0, 1] = V
    bad = bad.to(dev)
    pbuf, pview, _ = _place(dev, c["logits"], False)
    prow = _rows2d(pbuf, B, S, V)
    _, lse = _forward(KH, prow, chunks, c["ids_all"][0].to(dev), torch.empty((3, B, T), dtype=F32, device=dev))
    want = K.label_logprob_bwd(g, pview, lse, bad)
    for c0, c1 in chunks:
        KH.head_dlogits_chunk(g, prow[:, c0:c1], c0, V, lse, bad)
    assert torch.equal(_bits(pview), _bits(want)) and bool((_bits(pview[0, 0]) == 0).all())


# ----------------------------------------------------------------------------------------------------------------- the composed path
_COMPOSED = {}


def _composed_case(KH, dev, B, S, D, V, step):
    """h ~ N(0, 1), W ~ N(0, 1 / sqrt(D)), random labels and token weights; the oracle's logits are the concatenation of ``head_chunk_logits`` outputs (that GEMM is
    existing code and not under test).  Computed once per case."""
    key = (B, S, D, V, step)
    if key in _COMPOSED:
        return _COMPOSED[key]
    gen = torch.Generator().manual_seed(300 + B + S + D + V)
    h = torch.randn(B, S, D, generator=gen).to(BF16)
    w = (torch.randn(V, D, generator=gen) / D ** 0.5).to(BF16)
    ids = torch.randint(0, V, (B, S), generator=gen)
    g = torch.randn(B, S - 1, generator=gen)
    chunks = KH.head_chunks(B * S, V, step)
    hd, wd = h.to(dev), w.to(dev)
    parts = []
    for c0, c1 in chunks:
        scratch = torch.empty((B * S, (c1 - c0 + 7) // 8 * 8), dtype=BF16, device=dev)
        parts.append(KH.head_chunk_logits(hd.view(B * S, D), wd, c0, c1, scratch).clone())
    logits = torch.cat(parts, dim=1).view(B, S, V).cpu()
    logp64, lse64 = HO.chunked_logprobs(logits, ids, chunks, F64)
    logp32, lse32 = HO.chunked_logprobs(logits, ids, chunks, F32)
    _COMPOSED[key] = dict(h=h, w=w, ids=ids, g=g, chunks=chunks, logits=logits, logp64=logp64, logp32=logp32, logp16=GO.log_probs_per_token(logits, ids, BF16),
                          exact=HO.head_reference(h, w, ids, g, F64), flow16=HO.head_reference(h, w, ids, g, BF16), own=HO.own_flow_grads(logits, h, w, ids, g, chunks))
    return _COMPOSED[key]


@pytest.mark.parametrize("B,S,D,V,step", COMPOSED_CASES)
def test_composed_path(env, B, S, D, V, step):
    L, K, KH, G, dev = env
    c = _composed_case(KH, dev, B, S, D, V, step)
    h, w, ids, g = (c[k].to(dev) for k in ("h", "w", "ids", "g"))
    keep = [t.clone() for t in (h, w, ids, g)]
    report = []
    print(f"\n[head composed {B, S, D, V, step}] {len(c['chunks'])} chunks")
    logp, lse = KH.head_logprob_fwd(h, w, ids, step)
    assert logp.dtype == F32 and tuple(logp.shape) == (B, S - 1) == tuple(lse.shape)
    judge("logp", logp, c["logp16"], c["logp64"], report)
    _elementwise("logp", logp.cpu(), c["logp32"], c["logp64"], report)
    # another chunk width: the same bound against the same exact value
    for other in ({8: 16, 128: 256, None: 64}[step], V + 8 - V % 8):
        lp2, _ = KH.head_logprob_fwd(h, w, ids, other)
        judge(f"logp at vocab_chunk {other}", lp2, c["logp16"], c["logp64"], report)
        _elementwise(f"logp at vocab_chunk {other}", lp2.cpu(), c["logp32"], c["logp64"], report)
    dwbuf, dw = _guarded(dev, (V, D), BF16)
    dh = KH.head_logprob_bwd(g, h, w, lse, ids, step, dw_out=dw)
    torch.cuda.synchronize()
    assert _guards_intact(dwbuf) and not bool(torch.isnan(dw).any()) and not bool(torch.isnan(dh).any())
    assert dh.dtype == BF16 and tuple(dh.shape) == (B, S, D) and bool((_bits(dh[:, S - 1]) == 0).all()), "rows S - 1 of dh must be exact zeros"
    for t, k in zip((h, w, ids, g), keep):
        assert torch.equal(t, k), "an operand changed"
    for name, mine in (("dh", dh), ("dw", dw)):
        judge(name, mine.float(), c["flow16"][name].float(), c["exact"][name], report)
        _own_bound(name, mine.float(), c["own"][name], c["exact"][name], report)
    # two runs: the same bits
    logp_b, lse_b = KH.head_logprob_fwd(h, w, ids, step)
    dw_b = torch.empty_like(dw)
    dh_b = KH.head_logprob_bwd(g, h, w, lse_b, ids, step, dw_out=dw_b)
    assert torch.equal(_bits(logp_b), _bits(logp)) and torch.equal(_bits(lse_b), _bits(lse)) and torch.equal(_bits(dh_b), _bits(dh)) and torch.equal(_bits(dw_b), _bits(dw))
    # accumulation into a pre-filled gradient: the pre-fill plus the fresh result
    fill = (0.5 * torch.randn(V, D, generator=torch.Generator().manual_seed(9))).to(BF16)
    acc = fill.to(dev).clone()
    dh_c = KH.head_logprob_bwd(g, h, w, lse, ids, step, dw_out=acc, dw_accumulate=True)
    assert torch.equal(_bits(dh_c), _bits(dh))
    own_acc = (fill.float() + HO.own_flow_grads(c["logits"], c["h"], c["w"], c["ids"], c["g"], c["chunks"], dw_dtype=F32)["dw"]).to(BF16)
    _own_bound("dw accumulated", acc.float(), own_acc, fill.double() + c["exact"]["dw"], report)
    # an fp32 gradient buffer, and none at all
    dw32 = torch.empty((V, D), dtype=F32, device=dev)
    dh_d = KH.head_logprob_bwd(g, h, w, lse, ids, step, dw_out=dw32)
    _own_bound("dw fp32", dw32, HO.own_flow_grads(c["logits"], c["h"], c["w"], c["ids"], c["g"], c["chunks"], dw_dtype=F32)["dw"], c["exact"]["dw"], report)
    assert torch.equal(_bits(dh_d), _bits(dh)) and torch.equal(_bits(KH.head_logprob_bwd(g, h, w, lse, ids, step)), _bits(dh))
    _check(report)


def test_s_equal_one_is_empty_without_a_launch(env):
    L, K, KH, G, dev = env
    from llm_quest_amd.qwen.qwen3.qwen3_model import _OutHead

    head = _OutHead(torch.nn.Parameter(torch.zeros(16, 8, dtype=BF16, device=dev)))
    out = G.log_probs_per_token_from_hidden(torch.zeros(3, 1, 8, dtype=BF16, device=dev), head, torch.zeros(3, 1, dtype=I64, device=dev))
    assert out.shape == (3, 0) and out.dtype == F32


# ----------------------------------------------------------------------------------------------------------------- the loss
def test_loss_from_hidden_against_materialised_logits(env, fixture):
    """Case A of tests/golden/grpo_tiny.safetensors: hidden = its logits (emb_dim 40), head = the identity, which reproduces the logits bit for bit.  All five
    variants, with and without the off-policy mask.  The two paths' losses are two fp32 evaluations of the same log-probs (summed in fp64): 1e-6 relative,
    the figure the one-pass / two-pass comparison of tests/test_grpo_gpu.py holds."""
    L, K, KH, G, dev = env
    from llm_quest_amd.qwen.qwen3.qwen3_model import _OutHead

    t, meta = fixture
    report, pool = [], Pooled()
    dv = lambda x: x.to(dev)
    print("\n[loss from hidden, case A]")
    for variant in GO.VARIANTS:
        for m in (0, 1):
            a, key = GO.case_args(t, meta, "A", variant, 0, m)
            logits, ids, old, ref, adv, mask, ns, mg, _, _, delta = a
            B, S, V = logits.shape
            eye = torch.eye(V, dtype=BF16)
            assert torch.equal(torch.nn.functional.linear(logits.float(), eye.float()).to(BF16), logits)
            ha = (logits, eye, ids, old, ref, adv, mask, ns, mg, variant, False, delta)
            exact, flow16 = HO.head_loss_reference(*ha, F64, **SC), HO.head_loss_reference(*ha, BF16, **SC)
            own = GO.own_flow(*a)
            kw = dict(num_samples=ns, max_gen=mg, variant=variant, off_policy_delta=delta, **SC)
            head = _OutHead(torch.nn.Parameter(dv(eye).clone()))
            hid = dv(logits).clone().requires_grad_(True)
            keep = hid.detach().clone()
            loss = G.grpo_policy_loss_from_hidden(hid, head, dv(ids), dv(old), dv(ref), dv(adv), dv(mask), vocab_chunk=16, **kw)
            loss.backward()
            assert torch.equal(_bits(hid.detach()), _bits(keep)), "the hidden states must stay untouched"
            head2 = _OutHead(torch.nn.Parameter(dv(eye).clone()))
            hid2 = dv(logits).clone().requires_grad_(True)
            made = head2(hid2)
            assert torch.equal(_bits(made.detach()), _bits(dv(logits))), "the identity head must reproduce the fixture's logits"
            loss2 = G.grpo_policy_loss(made, dv(ids), dv(old), dv(ref), dv(adv), dv(mask), inplace=False, **kw)
            loss2.backward()
            rel = abs(float(loss) - float(loss2)) / abs(float(loss2))
            print(f"  {key}: from hidden {float(loss):.8f}  materialised {float(loss2):.8f}  relative {rel:.3e}")
            if not rel <= 1e-6:
                report.append(f"{key}: loss from hidden {float(loss)} against materialised {float(loss2)}: {rel:.3e} > 1e-6")
            judge(f"{key} loss", loss.detach().cpu(), flow16["loss"].float(), exact["loss"], report)
            pool.add("loss", loss, own["loss"], exact["loss"])
            for name, mine, theirs in (("dh", hid.grad, hid2.grad), ("dw", head.weight.grad, head2.weight.grad)):
                judge(f"{key} {name}", mine.float(), flow16[name].float(), exact[name], report)
                print(f"  {key} {name}: against the materialised path {GO.rel_l2(mine.cpu(), theirs.cpu()):.3e}")
            with torch.no_grad():
                l0 = G.grpo_policy_loss_from_hidden(hid.detach(), head, dv(ids), dv(old), dv(ref), dv(adv), dv(mask), vocab_chunk=16, **kw)
            assert l0.grad_fn is None and torch.equal(_bits(l0.reshape(1)), _bits(loss.detach().reshape(1))), "no-grad mode returns the forward's loss"
    pool.check(report)
    _check(report)


# ----------------------------------------------------------------------------------------------------------------- memory
def test_peak_memory_stays_below_a_quarter_of_the_logits(env):
    """B S = 4 x 256, D = 128, V = 32 768, vocab_chunk = 2 048: forward + backward may raise ``max_memory_allocated`` by less than a quarter of the logits'
    64 MiB above the level in front of the forward (the weight's gradient already attached).  The budget is derived: 4 MiB of chunk scratch, 0.5 MiB of
    fp32 dH, 0.25 MiB of bf16 dh, the state, at most one transposed weight chunk.  The materialised path must rise by the logits' bytes at least, which
    shows that the measurement sees what it should."""
    L, K, KH, G, dev = env
    from llm_quest_amd.qwen.qwen3.qwen3_model import _OutHead

    B, S, D, V, step = 4, 256, 128, 32768, 2048
    gen = torch.Generator().manual_seed(0)
    head = _OutHead(torch.nn.Parameter((torch.randn(V, D, generator=gen) / D ** 0.5).to(BF16).to(dev)))
    hid = torch.randn(B, S, D, generator=gen).to(BF16).to(dev).requires_grad_(True)
    ids = torch.randint(0, V, (B, S), generator=gen).to(dev)
    mask = torch.ones(B, S - 1, dtype=torch.bool, device=dev)
    adv = torch.tensor([1.0, -1.0, 0.5, -0.5], device=dev)
    with torch.no_grad():
        old = G.log_probs_per_token_from_hidden(hid, head, ids, step)
    kw = dict(num_samples=2, min_clip=0.2, max_clip=0.2, beta=0.1, max_gen=S)
    chunked = lambda: G.grpo_policy_loss_from_hidden(hid, head, ids, old, old, adv, mask, vocab_chunk=step, **kw).backward()
    whole = lambda: G.grpo_policy_loss(head(hid), ids, old, old, adv, mask, **kw).backward()
    rises = {}
    for name, fn in (("chunked", chunked), ("materialised", whole)):
        fn()  # warm-up: the GEMMs' split-K workspace, the arena's gradient and hid.grad exist from here on
        torch.cuda.synchronize()
        assert head.weight.grad is not None and hid.grad is not None
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        fn()
        torch.cuda.synchronize()
        rises[name] = torch.cuda.max_memory_allocated(dev) - base
    logits_bytes = B * S * V * 2
    print(f"\n[memory] logits {logits_bytes / 2**20:.1f} MiB; rise chunked {rises['chunked'] / 2**20:.2f} MiB, materialised {rises['materialised'] / 2**20:.2f} MiB")
    assert rises["materialised"] >= logits_bytes, "the measurement does not see the materialised logits"
    assert rises["chunked"] < logits_bytes // 4, f"the chunked path rose by {rises['chunked']} bytes, a quarter of the logits is {logits_bytes // 4}"


# ----------------------------------------------------------------------------------------------------------------- a tiny model
@pytest.mark.parametrize("variant", ["grpo", "gspo"])
def test_tiny_qwen3_takes_a_policy_gradient_step_from_hidden(env, variant):
    """``label_log_probs`` is ``forward_hidden`` + ``log_probs_per_token_from_hidden`` bit for bit; ``loss.backward()`` through ``grpo_policy_loss_from_hidden`` gives
    every parameter (the tied embedding included) the bits that the launcher's own dh and dW, fed by hand on a second forward, give; an SGD step then changes the
    weights and leaves them finite."""
    L, K, KH, G, dev = env
    from llm_quest_amd.ops import arena_for
    from llm_quest_amd.qwen.qwen3.qwen3_model import Qwen3Model

    torch.manual_seed(0)
    model = Qwen3Model(dict(TINY_QWEN)).to(dev).train()
    B, S, ns, step = 4, 16, 2, 128
    ids = torch.randint(0, TINY_QWEN["vocab_size"], (B, S), generator=torch.Generator().manual_seed(1)).to(dev)
    mask = torch.ones(B, S - 1, dtype=torch.bool)
    mask[:, :5] = False
    mask[1, 12:] = False
    mask = mask.to(dev)
    adv = torch.tensor([1.0, -1.0, 0.5, -0.5], device=dev)
    with torch.no_grad():
        old = model.label_log_probs(ids, vocab_chunk=step)
        direct = G.log_probs_per_token_from_hidden(model.forward_hidden(ids), model.out_head, ids, step)
        assert old.dtype == F32 and tuple(old.shape) == (B, S - 1) and torch.equal(_bits(old), _bits(direct))
        whole = G.log_probs_per_token(model(ids), ids)
        print(f"\n[tiny qwen3 {variant}] label_log_probs against log_probs_per_token(model(ids)): worst {float((old - whole).abs().max()):.3e}")
        noise = torch.Generator().manual_seed(2)
        ref = (old + 0.1 * torch.randn(old.shape, generator=noise).to(dev)).contiguous()
        old = (old + 0.1 * torch.randn(old.shape, generator=noise).to(dev)).contiguous()
    args = (0.2, 0.2, 0.1, ns, S, variant, False)
    model.zero_grad(set_to_none=True)
    loss = G.grpo_policy_loss_from_hidden(model.forward_hidden(ids), model.out_head, ids, old, ref, adv, mask, ns, 0.2, 0.2, 0.1, max_gen=S, variant=variant,
                                          vocab_chunk=step)
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    got = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    assert len(got) == len(list(model.named_parameters())) and all(bool(torch.isfinite(v.float()).all()) for v in got.values())
    # the launcher's own dh and dW, fed by hand on a second forward
    model.zero_grad(set_to_none=True)
    hidden = model.forward_hidden(ids)
    w = model.out_head.weight
    logp, lse = KH.head_logprob_fwd(hidden.detach(), w.detach(), ids, step)
    _, dlogp, _, _ = K.token_loss(logp, old, ref, adv, mask, *args)
    view, acc = arena_for(model.out_head).grad_target(w)
    dh = KH.head_logprob_bwd(dlogp, hidden.detach(), w.detach(), lse, ids, step, dw_out=view, dw_accumulate=acc)
    hidden.backward(dh)
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.equal(_bits(p.grad), _bits(got[n])), f"{n}: gradient bits differ"
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    opt.step()
    torch.cuda.synchronize()
    changed = sum(int(not torch.equal(p.detach(), before[n])) for n, p in model.named_parameters())
    assert changed > 0 and all(bool(torch.isfinite(p.float()).all()) for p in model.parameters())
