"""The GRPO kernels on the GPU against the fp64 restatement (tests/grpo_oracle.py) and the reference's own runs in tests/golden/grpo_tiny.safetensors.

Two yardsticks, both fixed when these kernels were added: the project's rule ``test_deepseek_moe_gpu.judge`` (the kernel may be at most 1.5 x as
far from fp64 as the reference's bf16 flow), and the distance of a CPU restatement of the kernel's own flow (fp32 throughout, the logits' gradient rounded to bf16
once) -- 4 x element-wise for the log-probs (the factor is for the fast exponential and the different summation order), 1.5 x in relative L2 for everything else.
The shapes are the smallest that cross an edge of the kernels (the 8-element chunk, the 8 192-element step of the register form, its two widths, more
rows than one block), not the workload's.  Every figure is printed before it is asserted (run with ``-s``)."""

import pytest
import torch

import grpo_oracle as GO
from test_deepseek_moe_gpu import judge

pytestmark = pytest.mark.gpu

BF16, F32, F64, I64 = torch.bfloat16, torch.float32, torch.float64, torch.int64
NAN = float("nan")
GUARD = 4096  # sentinel elements in front of and behind every operand
LOGPROB_CASES = [(1, 2, 1), (2, 3, 7), (2, 5, 8), (3, 4, 9), (2, 3, 1000), (1, 3, 8192), (1, 3, 8200), (2, 3, 50304), (1, 3, 151936)]
STRIDED = (2, 3, 1000)  # this case gets a batch stride larger than S * pitch and a pitch larger than V (the ``keep_rows`` view the models return)
SC = dict(min_clip=GO.MIN_CLIP, max_clip=GO.MAX_CLIP, beta=GO.BETA)


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from llm_quest_amd import _lib, kernels_grpo
    from llm_quest_amd.alignment.rlhf_grpo import grpo_engine

    _lib.load()
    return _lib, kernels_grpo, grpo_engine, torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fixture():
    return GO.load_fixture()


def _check(report):
    assert not report, "\n".join(report)


def _own_bound(name, mine, own, exact, report, factor=1.5):
    """``mine`` may be at most ``factor`` x as far from ``exact`` (relative L2) as the CPU restatement of the kernel's own flow."""
    mine, own, exact = mine.detach().cpu(), own.detach().cpu(), exact.detach().cpu()
    got, floor = GO.rel_l2(mine, exact), GO.rel_l2(own, exact)
    print(f"  {name}: kernel {got:.3e}  own flow {floor:.3e}  bound {factor * floor:.3e}")
    if not got <= factor * floor:
        report.append(f"{name}: {got:.3e} > {factor} x own flow {floor:.3e}")


class Pooled:
    """The own-flow bound for quantities of a few numbers (the scalar loss, a mean KL per sequence, the log-prob gradients of a 2 x 3 case).  An fp32 result
    cannot be held to 1.5 x the distance of ONE other fp32 computation of a single number: that distance is below half an ulp whenever the restatement's roundings
    happen to cancel (1.2e-9 for the dapo loss of the long case, against 3e-8 for half an ulp).  So the values of all configurations of a test are pooled
    per quantity and the relative L2 distance is taken over the pool -- the same metric and the same factor, on enough numbers to mean something."""

    def __init__(self):
        self.items = {}

    def add(self, name, mine, own, exact):
        m, o, e = self.items.setdefault(name, ([], [], []))
        m.append(mine.detach().cpu().double().flatten())
        o.append(own.detach().cpu().double().flatten())
        e.append(exact.detach().cpu().double().flatten())

    def check(self, report):
        for name, (m, o, e) in self.items.items():
            _own_bound(f"{name} (pooled over {len(m)} configurations)", torch.cat(m), torch.cat(o), torch.cat(e), report)


# ----------------------------------------------------------------------------------------------------------------- log-prob rows
def _border_labels(V):
    """0, V - 1 and both sides of every 8-element and every 8 192-element border that V has."""
    s = {0, V - 1}
    for step in (8, 8192):
        for k in range(step, V, step):
            s.update((k - 1, k))
    return sorted(s)


_CASES = {}


def _logprob_case(B, S, V):
    """Logits with the special rows, label sets that cover every border, and the three CPU flows of the log-probs; computed once per shape."""
    key = (B, S, V)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(1000 + B + 10 * S + V)
    logits = (3.0 * torch.randn(B, S, V, generator=g)).to(BF16)
    T = S - 1
    rows = [(b, s) for b in range(B) for s in range(T)]
    kinds = {}
    for (b, s), kind in zip(rows, ("equal", "pm120", "half_inf")):  # as many of the three special rows as the case has rows
        kinds[(b, s)] = kind
        if kind == "equal":
            logits[b, s] = 1.5
        elif kind == "pm120" and V >= 2:
            logits[b, s] = torch.where(torch.arange(V) % 2 == 0, 120.0, -120.0).to(BF16)
        elif kind == "half_inf" and V >= 2:
            logits[b, s, torch.arange(V) % 2 == 1] = float("-inf")
    cands = _border_labels(V)
    finite = [c for c in cands if c % 2 == 0] or [0]  # the row with -inf on the odd elements keeps a finite label
    n = len(rows)
    sets = []
    for i in range(0, len(cands), n):
        ids = torch.randint(0, V, (B, S), generator=g)
        for j, (b, s) in enumerate(rows):
            c = cands[(i + j) % len(cands)]
            if kinds.get((b, s)) == "half_inf" and c % 2 == 1:
                c = finite[(i + j) % len(finite)]
            ids[b, s + 1] = c
        sets.append(ids)
    ids_all = torch.stack(sets)  # [runs, B, S]
    x64 = logits[:, :-1].double()
    lse64 = torch.logsumexp(x64, dim=-1)
    x32 = logits[:, :-1].float()
    lse32 = torch.logsumexp(x32, dim=-1)
    lab = ids_all[:, :, 1:]
    logp64 = x64.unsqueeze(0).expand(len(sets), -1, -1, -1).gather(-1, lab.unsqueeze(-1)).squeeze(-1) - lse64
    logp32 = x32.unsqueeze(0).expand(len(sets), -1, -1, -1).gather(-1, lab.unsqueeze(-1)).squeeze(-1) - lse32
    logp16 = torch.stack([GO.log_probs_per_token(logits, ids, BF16) for ids in sets[:4]])
    _CASES[key] = dict(logits=logits, ids_all=ids_all, lse64=lse64, lse32=lse32, logp64=logp64, logp32=logp32, logp16=logp16, kinds=kinds)
    return _CASES[key]


def _place(dev, logits, strided):
    """The logits inside a NaN-filled device buffer with guards; returns (buffer, view, bool map of the elements the view covers)."""
    B, S, V = logits.shape
    pitch = (V + 7) // 8 * 8 + (24 if strided else 0)
    bstride = S * pitch + (5 * 8 if strided else 0)
    buf = torch.full((2 * GUARD + B * bstride,), NAN, dtype=BF16, device=dev)
    view = buf.as_strided((B, S, V), (bstride, pitch, 1), GUARD)
    view.copy_(logits.to(dev))
    covered = torch.zeros(buf.shape, dtype=torch.bool, device=dev)
    covered.as_strided((B, S, V), (bstride, pitch, 1), GUARD).fill_(True)
    return buf, view, covered


def _guarded(dev, shape, dtype=F32):
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((2 * GUARD + n,), NAN, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


def _guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


@pytest.mark.parametrize("B,S,V", LOGPROB_CASES)
def test_label_logprob_forward(env, B, S, V):
    L, K, G, dev = env
    c = _logprob_case(B, S, V)
    strided = (B, S, V) == STRIDED
    buf, view, _ = _place(dev, c["logits"], strided)
    before = buf.clone()
    runs, T = c["ids_all"].shape[0], S - 1
    ids_dev = c["ids_all"].to(dev)
    out_buf, out = _guarded(dev, (runs, 2, B, T))
    L.require_gpu(view, ids_dev, out)
    for r in range(runs):
        L.call("mi355_label_logprob_fwd", B, S, V, L.ptr(view), view.stride(0), view.stride(1), L.ptr(ids_dev[r]), L.ptr(out[r, 0]), L.ptr(out[r, 1]))
    again_buf, again = _guarded(dev, (2, B, T))
    L.call("mi355_label_logprob_fwd", B, S, V, L.ptr(view), view.stride(0), view.stride(1), L.ptr(ids_dev[0]), L.ptr(again[0]), L.ptr(again[1]))
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf), _bits(before)), "the forward changed the logits or their surroundings"
    assert _guards_intact(out_buf) and _guards_intact(again_buf), "a byte outside the outputs changed"
    assert not bool(torch.isnan(out).any()), "a sentinel survived in an output"
    assert torch.equal(_bits(again), _bits(out[0])), "two runs differ"
    logp, lse = out[:, 0].cpu(), out[:, 1].cpu()
    report = []
    print(f"\n[logprob fwd {B, S, V}] {runs} label sets")
    judge("logp", logp[:4], c["logp16"], c["logp64"][:4], report)
    judge("lse", lse[0], GO.lse_per_token(c["logits"], BF16), c["lse64"], report)
    for name, mine, own, exact in (("logp", logp, c["logp32"], c["logp64"]), ("lse", lse[0], c["lse32"], c["lse64"])):
        bound = 4.0 * float((own.double() - exact).abs().max())
        worst = float((mine.double() - exact).abs().max())
        print(f"  {name}: element-wise worst {worst:.3e}  bound 4 x fp32 restatement {bound:.3e}")
        if not worst <= bound:
            report.append(f"{name}: element-wise {worst:.3e} > {bound:.3e}")
    # the public function (padded copy where the pitch needs it) gives the same bits
    pub = G.log_probs_per_token(c["logits"].to(dev), ids_dev[0])
    assert pub.dtype == F32 and torch.equal(_bits(pub), _bits(out[0, 0])), "log_probs_per_token differs from the raw launch"
    assert torch.equal(G.log_probs_per_token_optimized(c["logits"].to(dev), ids_dev[0]), pub)
    # a label outside [0, V): NaN for its token only
    for bad_label in (-1, V):
        bad = ids_dev[0].clone()
        bad[B - 1, 1] = bad_label
        lp = G.log_probs_per_token(c["logits"].to(dev), bad)
        nan = torch.isnan(lp)
        assert bool(nan[B - 1, 0]) and int(nan.sum()) == 1, "an out-of-range label must give NaN for its token only"
        keep = ~nan
        assert torch.equal(_bits(lp)[keep], _bits(pub)[keep])
    _check(report)


@pytest.mark.parametrize("B,S,V", LOGPROB_CASES)
def test_label_logprob_backward(env, B, S, V):
    L, K, G, dev = env
    c = _logprob_case(B, S, V)
    strided = (B, S, V) == STRIDED
    T = S - 1
    gen = torch.Generator().manual_seed(7 + V)
    g = torch.randn(B, T, generator=gen)
    runs = c["ids_all"].shape[0]
    report = []
    print(f"\n[logprob bwd {B, S, V}]")
    for r in sorted({0, 1 % runs, runs // 2, runs - 1}):  # label sets that hold element 0, the first borders, the middle ones and V - 1
        ids = c["ids_all"][r]
        exact = GO.logprob_grad(c["logits"], ids, g, F64)
        own = GO.logprob_grad(c["logits"], ids, g, F32).to(BF16)
        flow16 = GO.logprob_grad(c["logits"], ids, g, BF16)
        buf, view, cov = _place(dev, c["logits"], strided)
        before = buf.clone()
        obuf, oview, ocov = _place(dev, torch.full((B, S, V), NAN, dtype=BF16), strided)
        obefore = obuf.clone()
        lse_k = K.label_logprob_fwd(view, ids.to(dev))[1]
        out = K.label_logprob_bwd(g.to(dev), view, lse_k, ids.to(dev), out=oview)
        torch.cuda.synchronize()
        assert torch.equal(_bits(buf), _bits(before)), "the out-of-place backward changed the logits"
        assert torch.equal(_bits(obuf)[~ocov], _bits(obefore)[~ocov]), "a byte outside the output changed"
        assert not bool(torch.isnan(oview).any()), "a sentinel survived in the output"
        assert bool((_bits(oview[:, S - 1]) == 0).all()), "row S - 1 must be exact zeros"
        fresh = K.label_logprob_bwd(g.to(dev), view, lse_k, ids.to(dev))
        assert torch.equal(_bits(fresh), _bits(oview)), "two runs differ"
        K.label_logprob_bwd(g.to(dev), view, lse_k, ids.to(dev), out=view)  # in place
        torch.cuda.synchronize()
        assert torch.equal(_bits(view), _bits(oview)), "in place differs from out of place"
        assert torch.equal(_bits(buf)[~cov], _bits(before)[~cov]), "the in-place backward changed a byte outside the logits"
        judge(f"dlogits[set {r}]", oview.float(), flow16, exact, report)
        _own_bound(f"dlogits[set {r}]", oview.float(), own, exact, report)
    # through autograd: the node writes into a fresh buffer, the logits stay the caller's
    x = c["logits"].to(dev).requires_grad_(True)
    keep = x.detach().clone()
    (G.log_probs_per_token(x, c["ids_all"][0].to(dev)) * g.to(dev)).sum().backward()
    assert torch.equal(_bits(x.detach()), _bits(keep)) and x.grad.shape == x.shape
    _own_bound("autograd dlogits", x.grad.float(), GO.logprob_grad(c["logits"], c["ids_all"][0], g, F32).to(BF16), GO.logprob_grad(c["logits"], c["ids_all"][0], g, F64), report)
    _check(report)


def test_s_equal_one_is_empty_without_a_launch(env):
    L, K, G, dev = env
    out = G.log_probs_per_token(torch.zeros(3, 1, 16, dtype=BF16, device=dev), torch.zeros(3, 1, dtype=I64, device=dev))
    assert out.shape == (3, 0) and out.dtype == F32


def test_large_offsets(env):
    """A 4.4 GB bf16 allocation: the operand of the first part is its last 3 rows of V = 8200 (every byte offset from the allocation's base is past 2^32); the second
    part addresses the first and the last 3 rows as ONE batch of two through a batch stride past 2^31 elements, so the kernels' own row arithmetic has to be
    64-bit.  Only those rows are touched."""
    L, K, G, dev = env
    V, S = 8200, 3
    n = 2_200_000_000 + 8
    free, _ = torch.cuda.mem_get_info()
    if free < 3 * n:
        pytest.skip(f"needs {3 * n} bytes of device memory, torch.cuda.mem_get_info() reports {free} free")
    big = torch.empty(n, dtype=BF16, device=dev)
    last = n - S * V
    assert last % 8 == 0 and last * 2 > 1 << 32
    c = _logprob_case(1, 3, 8200)
    gen = torch.Generator().manual_seed(5)
    two = (3.0 * torch.randn(2, S, V, generator=gen)).to(BF16)
    ids2 = torch.randint(0, V, (2, S), generator=gen)
    g2 = torch.randn(2, S - 1, generator=gen)
    tail = big.as_strided((1, S, V), (S * V, V, 1), last)
    tail.copy_(c["logits"].to(dev))
    ids = c["ids_all"][0].to(dev)
    logp, lse = K.label_logprob_fwd(tail, ids)
    small = c["logits"].to(dev)
    logp_s, lse_s = K.label_logprob_fwd(small, ids)
    assert torch.equal(_bits(logp), _bits(logp_s)) and torch.equal(_bits(lse), _bits(lse_s))
    g = torch.randn(1, S - 1, generator=gen).to(dev)
    want = K.label_logprob_bwd(g, small, lse_s, ids)
    K.label_logprob_bwd(g, tail, lse, ids, out=tail)
    assert torch.equal(_bits(tail), _bits(want))
    both = big.as_strided((2, S, V), (last, V, 1), 0)
    assert both.stride(0) > 1 << 31
    both.copy_(two.to(dev))
    small2 = two.to(dev)
    logp, lse = K.label_logprob_fwd(both, ids2.to(dev))
    logp_s, lse_s = K.label_logprob_fwd(small2, ids2.to(dev))
    assert torch.equal(_bits(logp), _bits(logp_s)) and torch.equal(_bits(lse), _bits(lse_s))
    old = (logp_s + 0.3 * torch.randn(2, S - 1, generator=gen).to(dev)).contiguous()
    adv = torch.tensor([1.0, -1.0], device=dev)
    mask = torch.ones(2, S - 1, dtype=torch.bool, device=dev)
    l_s, _, lp_s, d_s = K.logits_loss(small2, ids2.to(dev), old, old, adv, mask, 0.2, 0.2, 0.1, 2)
    l_b, _, lp_b, _ = K.logits_loss(both, ids2.to(dev), old, old, adv, mask, 0.2, 0.2, 0.1, 2, out=both)
    torch.cuda.synchronize()
    assert torch.equal(_bits(l_b.reshape(1)), _bits(l_s.reshape(1))) and torch.equal(_bits(lp_b), _bits(lp_s)) and torch.equal(_bits(both), _bits(d_s))
    del big


# ----------------------------------------------------------------------------------------------------------------- the per-token chain
_SYN = {}


def _synthetic():
    """T = 1030, B = 4 under the fixture's conditions (first seed that meets them), with its delta; crosses the 256-token steps of the per-sequence sums."""
    if _SYN:
        return _SYN
    for seed in range(64):
        inp = GO.synthetic_logp(4, 1030, seed)
        pol, old, ref, adv, mask = (inp[k] for k in ("pol", "old", "ref", "adv", "mask"))
        r = torch.exp(pol.double() - old.double())
        if bool((((r - (1 - GO.MIN_CLIP)).abs() < 1e-3) | ((r - (1 + GO.MAX_CLIP)).abs() < 1e-3)).any()) or bool((adv == 0).any()):
            continue
        means = [GO.off_policy_mask(GO.k3(pol.double(), ref.double(), rho), adv.double(), mask, 0.0)[1] for rho in (None, r)]
        neg = [float(v) for v, a in zip(means[0], adv) if a < 0]
        lower = [float(v) for v in means[0] if float(v) < max(neg)]
        if not lower:
            continue
        delta = 0.5 * (max(lower) + max(neg))
        masks = [GO.off_policy_mask(GO.k3(pol.double(), ref.double(), rho), adv.double(), mask, delta)[0] for rho in (None, r)]
        if any(bool(m.all()) or not bool(m.any()) for m in masks) or any(bool(((mk - delta).abs() < 1e-3).any()) for mk in means):
            continue
        _SYN.update(inp, delta=delta, seed=seed, num_samples=2, max_gen=1030)
        return _SYN
    raise AssertionError("no seed meets the conditions")


def _token_case(fixture, case, variant):
    """(pol, old, ref, adv, mask, num_samples, max_gen, delta) on the CPU; the fixture's policy log-probs are the fp32 rounding of the fp64 ones."""
    if case == "S":
        s = _synthetic()
        return s["pol"], s["old"], s["ref"], s["adv"], s["mask"], s["num_samples"], s["max_gen"], s["delta"]
    t, meta = fixture
    args, _ = GO.case_args(t, meta, case, variant, 0, 1)
    pol = GO.log_probs_per_token(args[0], args[1], F64).float()
    return pol, args[2], args[3], args[4], args[5], args[6], args[7], args[10]


@pytest.mark.parametrize("case", ["A", "B", "S"])
def test_token_loss(env, fixture, case):
    L, K, G, dev = env
    report, pool = [], Pooled()
    for variant, u, m in GO.configs():
        pol, old, ref, adv, mask, ns, mg, delta = _token_case(fixture, case, variant)
        print(f"\n[token loss {case} {variant} u{u} m{m}]")
        d = delta if m else None
        a = (pol, old, ref, adv, mask, ns, mg, variant, bool(u), d)
        exact, own, flow16 = GO.loss_and_dlogp(*a, F64), GO.loss_and_dlogp(*a, F32), GO.loss_and_dlogp(*a, BF16)
        first = None
        for mdt in (torch.bool, F32, I64):
            loss, dlogp, opm, mean_kl = K.token_loss(pol.to(dev), old.to(dev), ref.to(dev), adv.to(dev), mask.to(mdt).to(dev), SC["min_clip"], SC["max_clip"],
                                                     SC["beta"], ns, mg, variant, bool(u), d)
            got = (loss.reshape(1), dlogp, opm, mean_kl)
            if first is None:
                first = got
                again = K.token_loss(pol.to(dev), old.to(dev), ref.to(dev), adv.to(dev), mask.to(dev), SC["min_clip"], SC["max_clip"], SC["beta"], ns, mg,
                                     variant, bool(u), d)
                assert torch.equal(_bits(again[0].reshape(1)), _bits(got[0])) and torch.equal(_bits(again[1]), _bits(got[1])), "two runs differ"
                nograd = K.token_loss(pol.to(dev), old.to(dev), ref.to(dev), adv.to(dev), mask.to(dev), SC["min_clip"], SC["max_clip"], SC["beta"], ns, mg,
                                      variant, bool(u), d, want_grad=False)
                assert nograd[1] is None and torch.equal(_bits(nograd[0].reshape(1)), _bits(got[0]))
            else:
                for x, y in zip(first, got):
                    assert torch.equal(x, y), f"mask dtype {mdt} changes the result"
        loss, dlogp, opm, mean_kl = first
        tag = f"u{u} m{m}"
        assert torch.equal(opm.cpu(), exact["opm"]), f"{tag}: off-policy mask"
        for name, mine, key in (("loss", loss, "loss"), ("dlogp", dlogp, "dlogp"), ("mean_kl", mean_kl, "mean_kl")):
            judge(f"{variant} {tag} {name}", mine.cpu().reshape(exact[key].shape), flow16[key].float(), exact[key], report)
            pool.add(name, mine, own[key], exact[key])
        if case != "S":  # the reference's own fp32 run: the kernel may be as far from it as the two are allowed to be from fp64 together
            want = float(fixture[0][f"{case}.{variant}.u{u}.m{m}.loss32"])
            ex = float(exact["loss"])
            ref_floor, rel = abs(want - ex) / abs(ex), abs(float(loss) - want) / abs(ex)
            print(f"  {tag} loss against the reference's fp32 run: {rel:.3e}  (that run against fp64: {ref_floor:.3e})")
            if not (ref_floor <= 1e-4 and rel <= 1e-4):  # two fp32 evaluations of O(1) terms that cancel to O(1e-2): 6e-8 x a condition number of a few hundred
                report.append(f"{variant} {tag}: loss {float(loss)} against the reference's fp32 run {want}: {rel:.3e}; that run against fp64: {ref_floor:.3e}; bound 1e-4")
            assert torch.equal(opm.cpu(), fixture[0][f"{case}.{variant}.u{u}.m{m}.opm"].bool())
    pool.check(report)
    _check(report)


# ----------------------------------------------------------------------------------------------------------------- one pass against two passes
def _logits_case(fixture, case):
    if case == "W":  # (2, 5, 8200): the register form, more rows than sequences
        inp = GO.fixture_inputs(2, 5, 8200, 2, 11)
        return (inp["logits"], inp["ids"], inp["old"], inp["ref"], inp["adv"], inp["mask"], 2, 4)
    t, meta = fixture
    return GO.case_args(t, meta, case, "grpo", 0, 0)[0][:8]


@pytest.mark.parametrize("case", ["A", "B", "W"])
def test_one_pass_against_two_pass(env, fixture, case):
    L, K, G, dev = env
    logits, ids, old, ref, adv, mask, ns, mg = _logits_case(fixture, case)
    report, pool = [], Pooled()
    dv = lambda x: x.to(dev)
    for variant, u in [(v, u) for v in GO.TOKEN_LEVEL for u in (0, 1)]:
        print(f"\n[one pass / two pass {case} {variant} u{u}]")
        a = (logits, ids, old, ref, adv, mask, ns, mg, variant, bool(u), None)
        exact, own, flow16 = GO.loss_and_grads(*a, F64), GO.own_flow(*a), GO.loss_and_grads(*a, BF16)
        kw = dict(num_samples=ns, max_gen=mg, variant=variant, unbiased_kl_estimate=bool(u), **SC)
        results = {}
        for path in ("one", "two"):
            x = dv(logits).requires_grad_(True)
            keep = x.detach().clone()
            if path == "one":
                loss = G.grpo_policy_loss(x, dv(ids), dv(old), dv(ref), dv(adv), dv(mask), inplace=False, **kw)
            else:  # the two-pass path, as the reference-named functions compose it
                lp = G.log_probs_per_token(x, dv(ids))
                ratio = torch.exp(lp - dv(old))
                kl = G.kl_div_per_token(lp, dv(ref), policy_ratio=ratio if u else None)
                loss = G.GRPOLoss.compute(ratio, dv(adv), dv(mask), SC["min_clip"], SC["max_clip"], SC["beta"], kl, ns, max_gen=mg, variant=variant)
            loss.backward()
            assert torch.equal(_bits(x.detach()), _bits(keep)), f"{path}: inplace=False must leave the logits untouched"
            results[path] = (loss.detach().cpu(), x.grad.detach().cpu())
            judge(f"{variant} u{u} {path} loss", results[path][0], flow16["loss"].float(), exact["loss"], report)
            pool.add(f"{path} loss", results[path][0], own["loss"], exact["loss"])
            judge(f"{variant} u{u} {path} dlogits", results[path][1].float(), flow16["dlogits"].float(), exact["dlogits"], report)
            _own_bound(f"{variant} u{u} {path} dlogits", results[path][1].float(), own["dlogits"], exact["dlogits"], report)
        rel = abs(float(results["one"][0]) - float(results["two"][0])) / abs(float(results["two"][0]))
        print(f"  u{u} one pass against two pass, loss: {rel:.3e}")
        if not rel <= 1e-6:
            report.append(f"{variant} u{u}: the losses of the two paths differ by {rel:.3e} > 1e-6")
        # the kernels' two-pass path: bit-equal log-probs, the same loss bound, in place == out of place
        l1, _, lp1, d1 = K.logits_loss(dv(logits), dv(ids), dv(old), dv(ref), dv(adv), dv(mask), SC["min_clip"], SC["max_clip"], SC["beta"], ns, mg, variant, bool(u))
        lp2, lse2 = K.label_logprob_fwd(dv(logits), dv(ids))
        assert torch.equal(_bits(lp1), _bits(lp2)), "policy_logp of the two paths must be bit-equal"
        l2, dlogp, _, _ = K.token_loss(lp2, dv(old), dv(ref), dv(adv), dv(mask), SC["min_clip"], SC["max_clip"], SC["beta"], ns, mg, variant, bool(u))
        if not abs(float(l1) - float(l2)) <= 1e-6 * abs(float(l2)):
            report.append(f"u{u}: kernel losses {float(l1)} / {float(l2)}")
        d2 = K.label_logprob_bwd(dlogp, dv(logits), lse2, dv(ids))
        _own_bound(f"u{u} two-pass kernels dlogits", d2.float(), own["dlogits"], exact["dlogits"], report)
        consumed = dv(logits).clone()
        K.logits_loss(consumed, dv(ids), dv(old), dv(ref), dv(adv), dv(mask), SC["min_clip"], SC["max_clip"], SC["beta"], ns, mg, variant, bool(u), out=consumed)
        assert torch.equal(_bits(consumed), _bits(d1)), "in place differs from out of place"
        assert bool((_bits(d1[:, -1]) == 0).all()), "row S - 1 must be exact zeros"
        again = K.logits_loss(dv(logits), dv(ids), dv(old), dv(ref), dv(adv), dv(mask), SC["min_clip"], SC["max_clip"], SC["beta"], ns, mg, variant, bool(u))
        assert torch.equal(_bits(again[3]), _bits(d1)) and torch.equal(_bits(again[0].reshape(1)), _bits(l1.reshape(1))), "two runs differ"
        # inplace=True consumes the logits: they hold their gradient, which backward hands on
        x = dv(logits).clone().requires_grad_(True)
        y = x * 1  # a non-leaf, as a model's logits are
        loss = G.grpo_policy_loss(y, dv(ids), dv(old), dv(ref), dv(adv), dv(mask), **kw)
        loss.backward()
        assert torch.equal(_bits(y.detach()), _bits(d1)) and torch.equal(_bits(x.grad), _bits(d1))
        # no-grad mode: forward only, the same loss, nothing written
        with torch.no_grad():
            x = dv(logits).clone()
            keep = x.clone()
            l0 = G.grpo_policy_loss(x, dv(ids), dv(old), dv(ref), dv(adv), dv(mask), **kw)
        assert l0.grad_fn is None and torch.equal(_bits(x), _bits(keep)), "no-grad mode must not touch the logits"
        assert torch.equal(_bits(l0.reshape(1)), _bits(l2.reshape(1))), "no-grad mode returns the two-pass forward's loss"
    pool.check(report)
    _check(report)


def test_two_pass_paths_of_grpo_policy_loss(env, fixture):
    """gspo and the off-policy mask take the two-pass path; in place under the same flag."""
    L, K, G, dev = env
    t, meta = fixture
    report, pool = [], Pooled()
    dv = lambda x: x.to(dev)
    print("\n[grpo_policy_loss, two-pass]")
    for variant, u, m in (("gspo", 0, 0), ("gspo", 0, 1), ("grpo", 1, 1), ("sapo", 0, 1), ("dapo", 0, 1), ("dr_grpo", 1, 1)):
        a, key = GO.case_args(t, meta, "A", variant, u, m)
        logits, ids, old, ref, adv, mask, ns, mg, _, _, delta = a
        exact, own, flow16 = GO.loss_and_grads(*a, F64), GO.own_flow(*a), GO.loss_and_grads(*a, BF16)
        kw = dict(num_samples=ns, max_gen=mg, variant=variant, unbiased_kl_estimate=bool(u), off_policy_delta=delta, **SC)
        grads = []
        for inplace in (False, True):
            x = dv(logits).clone().requires_grad_(True)
            y = x * 1
            keep = y.detach().clone()
            loss = G.grpo_policy_loss(y, dv(ids), dv(old), dv(ref), dv(adv), dv(mask), inplace=inplace, **kw)
            loss.backward()
            assert inplace or torch.equal(_bits(y.detach()), _bits(keep))
            assert not inplace or torch.equal(_bits(y.detach()), _bits(x.grad))
            grads.append(x.grad.detach().cpu())
        assert torch.equal(_bits(grads[0]), _bits(grads[1]))
        judge(f"{key} loss", loss.detach().cpu(), flow16["loss"].float(), exact["loss"], report)
        pool.add("loss", loss, own["loss"], exact["loss"])
        judge(f"{key} dlogits", grads[0].float(), flow16["dlogits"].float(), exact["dlogits"], report)
        _own_bound(f"{key} dlogits", grads[0].float(), own["dlogits"], exact["dlogits"], report)
        want = t[key + ".dlogits32"]
        print(f"  {key} dlogits against the reference's fp32 run: {GO.rel_l2(grads[0][:, :-1].float(), want):.3e}")
    pool.check(report)
    _check(report)


# ----------------------------------------------------------------------------------------------------------------- the public functions
def test_public_functions_compose_to_grpo_policy_loss(env, fixture):
    """Composed as the reference's loop composes them (:1082-1111), every variant and flag of case A: the loss of ``grpo_policy_loss`` to 1e-6 relative, the
    logits' gradient by the own-flow bound; each intermediate against the reference's fp32 run."""
    L, K, G, dev = env
    t, meta = fixture
    report = []
    dv = lambda x: x.to(dev)
    print("\n[public functions, case A]")
    for variant, u, m in GO.configs():
        a, key = GO.case_args(t, meta, "A", variant, u, m)
        logits, ids, old, ref, adv, mask, ns, mg, _, _, delta = a
        exact, own = GO.loss_and_grads(*a, F64), GO.own_flow(*a)
        x = dv(logits).requires_grad_(True)
        lp = G.log_probs_per_token(x, dv(ids))
        if variant == "gspo":
            ratio = torch.exp(G.log_probs_per_seq(lp, dv(mask)) - G.log_probs_per_seq(dv(old), dv(mask)))
        else:
            ratio = torch.exp(lp - dv(old))
        kl = G.kl_div_per_token(lp, dv(ref), policy_ratio=ratio) if (u and variant != "gspo") else G.kl_div_per_token(lp, dv(ref))
        opm = G.off_policy_seq_mask(kl, dv(adv), dv(mask), delta=delta) if m else None
        loss = G.GRPOLoss.compute(policy_ratio=ratio, advantages=dv(adv), loss_mask=dv(mask), kl_div=kl, num_samples=ns, max_gen=mg, variant=variant,
                                  off_policy_mask=opm, **SC)
        loss.backward()
        y = dv(logits).requires_grad_(True)
        direct = G.grpo_policy_loss(y, dv(ids), dv(old), dv(ref), dv(adv), dv(mask), ns, max_gen=mg, variant=variant, unbiased_kl_estimate=bool(u),
                                    off_policy_delta=delta if m else None, inplace=False, **SC)
        direct.backward()
        rel = abs(float(loss) - float(direct)) / abs(float(direct))
        print(f"  {key}: composed against grpo_policy_loss, loss {rel:.3e}")
        if not rel <= 1e-6:
            report.append(f"{key}: composed loss {float(loss)} against grpo_policy_loss {float(direct)}: {rel:.3e} > 1e-6")
        _own_bound(f"{key} composed dlogits", x.grad.float(), own["dlogits"], exact["dlogits"], report)
        _own_bound(f"{key} direct dlogits", y.grad.float(), own["dlogits"], exact["dlogits"], report)
        for name, mine in (("policy_ratio", ratio), ("kl_div", kl)):
            d = GO.rel_l2(mine.detach().cpu(), t[f"{key}.{name}"])
            if not d <= 1e-5:
                report.append(f"{key}: {name} against the reference's fp32 run: {d:.3e} > 1e-5")
        if m:
            assert opm.shape == (logits.shape[0], 1) and opm.dtype == torch.bool and torch.equal(opm.view(-1).cpu(), t[key + ".opm"].bool()), key
    # the smaller pieces against plain torch on the same device values
    a, key = GO.case_args(t, meta, "A", "grpo", 0, 0)
    pol = GO.log_probs_per_token(a[0], a[1], F64).float()
    r = torch.exp(pol - a[2]).requires_grad_(True)
    A_ = a[4].unsqueeze(-1)
    for name, fn, ref_fn in (("clipped", lambda q: G.GRPOLoss._compute_clipped_surrogate(q, dv(A_), SC["min_clip"], SC["max_clip"]),
                              lambda q: GO.clipped_surrogate(q, A_.double(), SC["min_clip"], SC["max_clip"])),
                             ("sapo", lambda q: G.GRPOLoss._compute_sapo_surrogate(q, dv(A_)), lambda q: GO.sapo_surrogate(q, A_.double()))):
        q = dv(r.detach()).requires_grad_(True)
        w = torch.randn(q.shape, generator=torch.Generator().manual_seed(3))
        out = fn(q)
        (out * dv(w)).sum().backward()
        q64 = r.detach().double().requires_grad_(True)
        out64 = ref_fn(q64)
        (out64 * w.double()).sum().backward()
        for what, mine, want in ((name, out, out64), (name + " grad", q.grad, q64.grad)):
            d = GO.rel_l2(mine.detach().cpu(), want.detach())
            print(f"  {what}: {d:.3e}")
            if not d <= 1e-6:
                report.append(f"{what}: {d:.3e} > 1e-6")
    lpt = (torch.randn(a[5].shape, generator=torch.Generator().manual_seed(4)) * a[5]).float()
    for variant in GO.TOKEN_LEVEL:
        q = dv(lpt).requires_grad_(True)
        out = G.GRPOLoss._aggregate(q, dv(a[5]), a[6], a[7], variant)
        out.backward()
        q64 = lpt.double().requires_grad_(True)
        out64 = GO.aggregate(q64, a[5], a[6], a[7], variant)
        out64.backward()
        for what, mine, want in ((f"aggregate {variant}", out, out64), (f"aggregate {variant} grad", q.grad, q64.grad)):
            d = GO.rel_l2(mine.detach().cpu(), want.detach())
            if not d <= 1e-6:
                report.append(f"{what}: {d:.3e} > 1e-6")
    seq = G.log_probs_per_seq(dv(pol), dv(a[5]))
    assert bool(torch.isnan(seq[4])) and int(torch.isnan(seq).sum()) == 1, "an empty mask gives NaN in log_probs_per_seq, as upstream"
    _check(report)


# ----------------------------------------------------------------------------------------------------------------- a tiny model
TINY_QWEN = dict(vocab_size=512, emb_dim=128, n_layers=2, n_heads=4, num_kv_groups=2, head_dim=128, hidden_dim=256, context_length=64, rope_base=1_000_000,
                 dtype=BF16, tie_embeddings=True)  # the small config of the Qwen3 tests (oracle/gen_golden.py), copied


@pytest.mark.parametrize("variant,delta", [("grpo", None), ("gspo", None), ("dapo", 0.05)])
def test_tiny_qwen3_takes_a_policy_gradient_step(env, variant, delta):
    """``loss.backward()`` through ``grpo_policy_loss`` gives every parameter the bits that feeding the kernel's own dlogits into ``logits.backward`` gives on a
    second forward; an optimizer step then changes the weights and leaves them finite."""
    L, K, G, dev = env
    from llm_quest_amd.qwen.qwen3.qwen3_model import Qwen3Model

    torch.manual_seed(0)
    model = Qwen3Model(dict(TINY_QWEN)).to(dev).train()
    B, S, ns = 4, 16, 2
    gen = torch.Generator().manual_seed(1)
    ids = torch.randint(0, TINY_QWEN["vocab_size"], (B, S), generator=gen).to(dev)
    mask = torch.ones(B, S - 1, dtype=torch.bool)
    mask[:, :5] = False
    mask[1, 12:] = False
    mask = mask.to(dev)
    adv = torch.tensor([1.0, -1.0, 0.5, -0.5], device=dev)
    with torch.no_grad():
        old = G.log_probs_per_token(model(ids), ids)
        noise = torch.Generator().manual_seed(2)
        ref = (old + 0.1 * torch.randn(old.shape, generator=noise).to(dev)).contiguous()
        old = (old + 0.1 * torch.randn(old.shape, generator=noise).to(dev)).contiguous()
    kw = dict(num_samples=ns, min_clip=0.2, max_clip=0.2, beta=0.1, max_gen=S, variant=variant, off_policy_delta=delta)
    model.zero_grad(set_to_none=True)
    logits = model(ids)
    loss = G.grpo_policy_loss(logits, ids, old, ref, adv, mask, **kw)
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    got = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    assert got and all(bool(torch.isfinite(v.float()).all()) for v in got.values())
    # the kernel's own dlogits (out of place, from identical logits), fed by hand
    model.zero_grad(set_to_none=True)
    logits2 = model(ids)
    x = logits2.detach().clone().requires_grad_(True)
    G.grpo_policy_loss(x, ids, old, ref, adv, mask, inplace=False, **kw).backward()
    logits2.backward(x.grad)
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        if p.grad is None:
            assert n not in got, n
            continue
        assert torch.equal(_bits(p.grad), _bits(got[n])), f"{n}: gradient bits differ"
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    opt.step()
    torch.cuda.synchronize()
    changed = sum(int(not torch.equal(p.detach(), before[n])) for n, p in model.named_parameters())
    assert changed > 0 and all(bool(torch.isfinite(p.float()).all()) for p in model.parameters())
