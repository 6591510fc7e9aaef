"""LatentMoE kernels (csrc/latent_moe.hip), ``Expert`` / ``SquaredReLU`` on their own and the layer on the GPU, against the plain-torch restatement
(tests/latent_moe_oracle.py) and the reference fixture (tests/golden/latent_moe_tiny*).

Tolerance: the project's 1.5x rule through ``test_deepseek_moe_gpu.judge`` and nothing else -- the relative L2 distance of a
kernel output to the fp64 restatement is at most 1.5 x the distance of the reference-dtype-flow restatement to the same fp64 result, with 2e-3 absolute
slack only where that floor is below 1e-2; where the fp64 result is identically zero the kernel is held to 1e-6 absolute per element.  Integer outputs,
selections and the bias update are compared exactly.  Where a selection enters a comparison, the restatement is evaluated on the selection the kernels
made (or both on a forced one).
"""

import json
import os

import pytest
import torch

import latent_moe_oracle as LO
from test_deepseek_moe_gpu import judge

pytestmark = pytest.mark.gpu
BF16, F32, I32, F64 = torch.bfloat16, torch.float32, torch.int32, torch.float64
ROUTE_CASES = [(1, 1, 1), (3, 3, 5), (12, 4, 70), (16, 8, 33), (65, 8, 64), (127, 8, 130), (128, 8, 96)]  # (E, k, T)
GLU_CASES = [(1, 8, 0), (33, 40, 8), (130, 96, 0), (515, 520, 24)]  # (R, F, pad)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


@pytest.fixture
def switch(monkeypatch):
    """Sets ``ops_moe.SEGMENTED`` for one test (the layers read it there, at call time)."""
    from llm_quest_amd import ops_moe

    return lambda on: monkeypatch.setattr(ops_moe, "SEGMENTED", bool(on))


def _kl():
    from llm_quest_amd import kernels_latmoe as KL

    return KL


# ----------------------------------------------------------------------------------------------------------------- router
_ROUTE = {}


def _route_bias(E, kind):
    if kind == "zero":
        return torch.zeros(E, dtype=BF16)
    g = torch.Generator().manual_seed(9 + E)  # of the size of the gaps between the probabilities; the fp32 ones are values bf16 cannot hold
    b = (0.05 * torch.randn(E, generator=g)).float()
    return b.to(BF16) if kind == "bf16" else b + 1e-4


def route_case(E, k, T, kind):
    """bf16 logits without a boundary tie in the biased key (the last row, when there is more than one, all equal), an upstream gradient and both flows
    of the restatement per scaling factor; computed once per case and shared (never modified) by the tests."""
    key = (E, k, T, kind)
    if key not in _ROUTE:
        b = _route_bias(E, kind)
        x = LO.logits_without_boundary_tie(T, E, k, b, seed=4000 + E + k + T)
        if T > 1:
            x[-1] = 0.5
        dw = torch.randn(T, k, generator=torch.Generator().manual_seed(77 + T))
        c = {"x": x, "b": b, "dw": dw}
        for sc in (1.0, 2.5):
            p, idx, w, s = LO.route(x, b, k, sc)
            p64, _, w64, s64 = LO.route(x, b, k, sc, dtype=F64, idx=idx)
            c[sc] = dict(idx=idx, ref=dict(p=p, w=w, s=s, dlogits=LO.route_bwd(x, b, k, sc, dw.to(BF16), idx=idx)),
                         exact=dict(p=p64, w=w64, s=s64, dlogits=LO.route_bwd(x, b, k, sc, dw, dtype=F64, idx=idx)))
        _ROUTE[key] = c
    return _ROUTE[key]


def _own_rounding_points(p, idx, w, s, scaling):
    """w and s exactly from the kernel's own p: s = bf16(slot-order fp32 sum), w = bf16(bf16(v / s) * scaling); an index that is no expert weighs 0."""
    E = p.shape[1]
    ok = (idx >= 0) & (idx < E)
    v = torch.where(ok, p.float().gather(1, idx.long().clamp(0, E - 1)), torch.zeros((), device=p.device))
    acc = torch.zeros(p.shape[0], device=p.device)
    for j in range(idx.shape[1]):
        acc = acc + v[:, j]
    assert torch.equal(s, acc.to(BF16).float()), "s is not bf16(the slot-order sum of the selected probabilities)"
    assert torch.equal(w, ((v / s.unsqueeze(1)).to(BF16).float() * scaling).to(BF16)), "w is not bf16(bf16(v / s) * scaling)"


@pytest.mark.parametrize("kind", ["zero", "bf16", "f32"])
@pytest.mark.parametrize("E,k,T", ROUTE_CASES)
def test_route_forward_and_backward_against_the_restatement(E, k, T, kind):
    KL = _kl()
    c = route_case(E, k, T, kind)
    x, b, dw = c["x"].cuda(), c["b"].cuda(), c["dw"].cuda()
    assert b.dtype == (F32 if kind == "f32" else BF16)
    bad = []
    for sc in (1.0, 2.5):
        r = c[sc]
        p, idx, w, s = KL.route_fwd(x, b, k, sc)
        assert torch.equal(idx.cpu().long(), r["idx"]), "the selected experts differ from the restatement's"
        if kind == "zero":
            assert torch.equal(idx.cpu().long(), LO.topk_lowest_index_first(r["ref"]["p"], k)[1])  # the plain top-k of p
            if T > 1:
                assert idx[-1].tolist() == list(range(k))  # all keys equal: the lower expert index wins
        srt = idx.sort(dim=1).values
        assert bool((srt[:, 1:] != srt[:, :-1]).all()) and int(idx.min()) >= 0 and int(idx.max()) < E
        for name, mine in (("p", p), ("w", w), ("s", s)):
            judge(f"{name} (scaling {sc})", mine, r["ref"][name], r["exact"][name], bad)
        _own_rounding_points(p, idx, w, s, sc)
        dl = KL.route_bwd(dw, s, idx, p, sc)
        judge(f"dlogits (scaling {sc})", dl, r["ref"]["dlogits"], r["exact"]["dlogits"], bad)
        sel = torch.zeros((T, E), dtype=torch.bool, device="cuda").scatter_(1, idx.long(), True)
        assert bool((dl[~sel] == 0).all()), "a sigmoid does not couple experts: dlogits is exactly zero at the experts that were not selected"
    # (scaling 2.5 from here on) a column slice of a wider buffer whose pad columns hold large values routes the same, forward and backward
    wide = torch.full((T, E + 25), 60.0, dtype=BF16, device="cuda")
    wide[:, 8 : 8 + E] = x
    p3, idx3, w3, s3 = KL.route_fwd(wide[:, 8 : 8 + E], b, k, 2.5)
    assert torch.equal(p3, p) and torch.equal(idx3, idx) and torch.equal(w3, w) and torch.equal(s3, s)
    dwide = torch.full((T, E + 25), 9.0, dtype=BF16, device="cuda")
    KL.route_bwd(dw, s, idx, p, 2.5, dlogits=dwide[:, 8 : 8 + E])
    assert torch.equal(dwide[:, 8 : 8 + E], dl) and bool((dwide[:, :8] == 9.0).all()) and bool((dwide[:, 8 + E :] == 9.0).all())
    # forced selection: the given experts, weighed with this call's own probabilities; the biases are not needed
    forced = ((idx.long() + 1) % E).flip(1).to(I32).contiguous() if E > k else idx.flip(1).contiguous()
    pf, idxf, wf, sf = KL.route_fwd(x, b, k, 2.5, forced_idx=forced)
    assert torch.equal(idxf, forced) and torch.equal(pf, p)
    _own_rounding_points(pf, idxf, wf, sf, 2.5)
    _, _, wr, sr = LO.route(c["x"], c["b"], k, 2.5, idx=forced.cpu().long())
    _, _, w64, s64 = LO.route(c["x"], c["b"], k, 2.5, dtype=F64, idx=forced.cpu().long())
    judge("forced w", wf, wr, w64, bad)
    judge("forced s", sf, sr, s64, bad)
    dlf = KL.route_bwd(dw, sf, idxf, pf, 2.5)
    judge("forced dlogits", dlf, LO.route_bwd(c["x"], c["b"], k, 2.5, c["dw"].to(BF16), idx=forced.cpu().long()),
          LO.route_bwd(c["x"], c["b"], k, 2.5, c["dw"], dtype=F64, idx=forced.cpu().long()), bad)
    if E > 1:  # an index that is no expert weighs 0 and gets no gradient
        off = forced.clone()
        off[:, 0] = torch.where(torch.arange(T, device="cuda") % 2 == 0, E, -1).to(I32)
        po, idxo, wo, so = KL.route_fwd(x, b, k, 2.5, forced_idx=off)
        assert torch.equal(idxo, off) and bool((wo[:, 0] == 0).all())
        if k > 1:
            _own_rounding_points(po, idxo, wo, so, 2.5)
            dlo = KL.route_bwd(dw, so, idxo, po, 2.5)
            sel = torch.zeros((T, E), dtype=torch.bool, device="cuda").scatter_(1, off[:, 1:].long(), True)
            assert bool(torch.isfinite(dlo.float()).all()) and bool((dlo[~sel] == 0).all())
    assert not bad, "\n".join(bad)


# ----------------------------------------------------------------------------------------------------------------- activation
_GLU = {}


def glu_case(R, F_, pad):
    key = (R, F_, pad)
    if key not in _GLU:
        g = torch.Generator().manual_seed(R + F_)
        gu = torch.randn(R, 2 * F_, generator=g).to(BF16)
        da = torch.randn(R, F_, generator=g).to(BF16)
        gate = gu[:, F_:]
        gate[torch.rand(R, F_, generator=g) < 0.1] = 0.0  # g == 0 planted: relu'(0) = 0 here as in torch
        gate[0, 0], gate[-1, -1] = 0.0, -0.0
        gate[0, 1 % F_ if F_ > 1 else 0] = -3.0
        a, dgu = LO.relu2_glu_grads(gu, da)
        a64, dgu64 = LO.relu2_glu_grads(gu, da, dtype=F64)
        _GLU[key] = dict(gu=gu, da=da, ref=(a, dgu), exact=(a64, dgu64))
    return _GLU[key]


@pytest.mark.parametrize("R,F_,pad", GLU_CASES)
def test_relu2_glu_forward_and_backward(R, F_, pad):
    KL = _kl()
    c = glu_case(R, F_, pad)
    SENT = 7.0
    wide = torch.full((R, 2 * F_ + pad + 8), SENT, dtype=BF16, device="cuda")  # the operands as column slices of wider buffers
    gu = wide[:, pad : pad + 2 * F_]
    gu.copy_(c["gu"])
    dwide = torch.full((R, F_ + pad), SENT, dtype=BF16, device="cuda")
    da = dwide[:, pad : pad + F_]
    da.copy_(c["da"])
    neg = (c["gu"][:, F_:] <= 0).cuda()
    assert bool(neg.any()) and bool((c["gu"][:, F_:] == 0).any()) and bool((c["gu"][:, F_:] < 0).any())

    def run():
        # guard rows above and below and pad columns left and right of both outputs, filled with a sentinel
        abuf = torch.full((R + 2, F_ + 16), SENT, dtype=BF16, device="cuda")
        dbuf = torch.full((R + 2, 2 * F_ + 16), SENT, dtype=BF16, device="cuda")
        a = KL.relu2_glu_fwd(gu, F_, out=abuf[1 : R + 1, 8 : 8 + F_])
        dgu = KL.relu2_glu_bwd(gu, da, F_, out=dbuf[1 : R + 1, 8 : 8 + 2 * F_])
        for buf, width in ((abuf, F_), (dbuf, 2 * F_)):
            assert bool((buf[0] == SENT).all()) and bool((buf[-1] == SENT).all()), "a guard row was written"
            assert bool((buf[:, :8] == SENT).all()) and bool((buf[:, 8 + width :] == SENT).all()), "a pad column was written"
        return a.contiguous(), dgu.contiguous()

    a, dgu = run()
    a2, dgu2 = run()
    assert torch.equal(a, a2) and torch.equal(dgu, dgu2), "two runs differ"
    assert bool((wide[:, :pad] == SENT).all()) and bool((wide[:, pad + 2 * F_ :] == SENT).all()) and torch.equal(gu.cpu(), c["gu"])  # inputs untouched
    assert bool((a[neg] == 0).all()), "a must be exactly zero where g <= 0"
    assert bool((dgu[:, F_:][neg] == 0).all()), "dg must be exactly zero where g <= 0"
    assert bool((dgu[:, :F_][neg] == 0).all())  # du = da * relu(g)^2
    bad = []
    judge("a", a, c["ref"][0], c["exact"][0], bad)
    judge("dgu", dgu, c["ref"][1], c["exact"][1], bad)
    judge("du", dgu[:, :F_], c["ref"][1][:, :F_], c["exact"][1][:, :F_], bad)
    judge("dg", dgu[:, F_:], c["ref"][1][:, F_:], c["exact"][1][:, F_:], bad)
    assert torch.equal(KL.relu2_glu_fwd(gu, F_), a) and torch.equal(KL.relu2_glu_bwd(gu, da, F_), dgu)  # the launchers' own outputs
    assert not bad, "\n".join(bad)


# ----------------------------------------------------------------------------------------------------------------- Expert and SquaredReLU alone
@pytest.mark.parametrize("input_dim", [16, 64])
def test_expert_on_its_own(input_dim):
    from llm_quest_amd.moe.nvidia_latent_moe import Expert

    T, hidden = 33, 40
    g = torch.Generator().manual_seed(input_dim)
    r = lambda *shape, scale: (scale * torch.randn(*shape, generator=g)).to(BF16)
    sd = {"lin1.weight": r(hidden, input_dim, scale=input_dim ** -0.5), "lin_gate.weight": r(hidden, input_dim, scale=input_dim ** -0.5),
          "lin2.weight": r(input_dim, hidden, scale=hidden ** -0.5)}
    x, dy = r(T, input_dim, scale=1.0), r(T, input_dim, scale=1.0)
    ex = Expert(dict(LO.FIXTURE_CFG), input_dim=input_dim, hidden_dim=hidden)
    ex.load_state_dict(sd)
    ex = ex.cuda()
    xg = x.view(1, T, input_dim).cuda().requires_grad_(True)
    y = ex(xg)
    y.backward(dy.view(1, T, input_dim).cuda())
    ops = [sd[n] for n in ("lin1.weight", "lin_gate.weight", "lin2.weight")]
    ref, exact = LO.expert_grads(x, *ops, dy), LO.expert_grads(x, *ops, dy, dtype=F64)
    mine = (y.view(T, input_dim), xg.grad.view(T, input_dim), ex.lin1.weight.grad, ex.lin_gate.weight.grad, ex.lin2.weight.grad)
    bad = []
    for name, m_, r_, e_ in zip(("out", "dx", "d lin1.weight", "d lin_gate.weight", "d lin2.weight"), mine, ref, exact):
        judge(name, m_, r_, e_, bad)
    with torch.no_grad():
        y2 = ex(xg)
    assert torch.equal(y2, y) and y2.grad_fn is None
    with pytest.raises(RuntimeError):
        y2.sum().backward()
    assert not bad, "\n".join(bad)


def test_squared_relu_on_its_own():
    from llm_quest_amd.moe.nvidia_latent_moe import SquaredReLU

    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 17, 24, generator=g).to(BF16)
    x[0, 0, :4] = torch.tensor([0.0, -0.0, -2.0, 3.0]).to(BF16)
    dy = torch.randn(2, 17, 24, generator=g).to(BF16)
    xg = x.cuda().requires_grad_(True)
    y = SquaredReLU()(xg)
    y.backward(dy.cuda())
    xr = x.clone().requires_grad_(True)
    yr = torch.square(torch.relu(xr))
    yr.backward(dy)
    x64 = x.double().requires_grad_(True)
    y64 = torch.square(torch.relu(x64))
    y64.backward(dy.double())
    assert torch.equal(y.cpu(), yr.detach()) and y[0, 0, :4].tolist() == [0.0, 0.0, 0.0, 9.0]  # one product, one rounding: the same bits
    assert bool((xg.grad.cpu()[x <= 0] == 0).all())
    bad = []
    judge("dx", xg.grad, xr.grad, x64.grad, bad)
    assert not bad, "\n".join(bad)


# ----------------------------------------------------------------------------------------------------------------- the layer on the fixture
@pytest.fixture(scope="module")
def fixture():
    return LO.load_fixture("latent_moe_tiny")


def _layer(name, t, forced=True):
    from llm_quest_amd.moe.nvidia_latent_moe import LatentMoE

    spec, pre = LO.FIXTURE_LAYERS[name], name + "."
    m = LatentMoE(dict(LO.FIXTURE_CFG), **spec["kwargs"])
    if spec["to_bf16"]:
        m = m.to(BF16)
    m.load_state_dict({n[len(pre + "sd."):]: v for n, v in t.items() if n.startswith(pre + "sd.")})
    m = m.cuda().train()
    if forced:
        m._forced_topk = t[pre + "topk_idxs"].cuda()
    return m


def _step(m, x):
    """One training forward + the fixture's loss + backward -> (out, dx, {name: gradient})."""
    xg = x.cuda().requires_grad_(True)
    out = m(xg)
    out.float().square().mean().backward()
    return out.detach(), xg.grad, {n: p.grad for n, p in m.named_parameters()}


@pytest.mark.parametrize("name", list(LO.FIXTURE_LAYERS))
def test_layer_on_the_fixture(name, fixture):
    t, spec, pre = fixture, LO.FIXTURE_LAYERS[name], name + "."
    E, k = spec["E"], spec["k"]
    x = t[pre + "in.x"]
    with open(os.path.join(LO.GOLDEN, "latent_moe_signatures.json")) as f:
        want = json.load(f)["state_dict"][name]
    # normal routing: the reference's selection on every robust token
    m = _layer(name, t, forced=False)
    sd = m.state_dict()
    assert set(sd) == set(want)
    for n, v in sd.items():
        assert list(v.shape) == want[n]["shape"] and str(v.dtype).replace("torch.", "") == want[n]["dtype"], (n, v.shape, v.dtype)
    assert m.biases.dtype == (BF16 if spec["to_bf16"] else F32)
    m(x.cuda())
    robust = t[pre + "robust"].bool()
    mine, ref = m._routed[0].cpu().long().sort(dim=1).values, t[pre + "topk_idxs"].long().sort(dim=1).values
    same = (mine == ref).all(dim=1)
    print(f"  {int(robust.sum())} of {robust.numel()} tokens robust; the selection agrees on {int(same.sum())}")
    assert int(robust.sum()) * 10 >= 9 * robust.numel() and bool(same[robust].all()), "a robust token selects other experts than the reference"
    assert torch.equal(m.biases.cpu(), LO.bias_update(t[pre + "sd.biases"], m._routed[1].cpu().long(), LO.RATE))  # the update from this forward's own counts
    # the reference's selection forced: counts and updated biases exact, output and every gradient under the 1.5x rule
    m = _layer(name, t)
    out, dx, grads = _step(m, x)
    assert torch.equal(m._routed[0].cpu(), t[pre + "topk_idxs"]) and torch.equal(m._routed[1].cpu(), t[pre + "counts"])
    assert m.biases.dtype == t[pre + "biases"].dtype and torch.equal(m.biases.cpu(), t[pre + "biases"]), "updated biases"
    assert m.max_vio.dim() == 0 and bool(torch.isfinite(m.max_vio))
    bad = []
    judge("out", out, t[pre + "out"], t[pre + "twin.out"], bad)
    judge("dx", dx, t[pre + "grad.x"], t[pre + "twin.grad.x"], bad)
    lo, hi = m._arena.grad.data_ptr(), m._arena.grad.data_ptr() + m._arena.grad.numel() * 2
    for n, g in grads.items():
        assert g is not None and lo <= g.data_ptr() < hi, n
        if pre + "grad." + n not in t:  # an expert that received no token: the reference leaves None, here an exactly zero gradient
            assert n.startswith("routed_experts.") and int(t[pre + "counts"][int(n.split(".")[1])]) == 0 and bool((g == 0).all()), n
            continue
        judge("d " + n, g, t[pre + "grad." + n], t[pre + "twin.grad." + n], bad)
    # eval(): the biases do not move; the no-grad forward gives the training forward's bits; no backward through it
    m.eval()
    before = m.biases.clone()
    with torch.no_grad():
        out2 = m(x.cuda())
    assert torch.equal(m.biases, before), "an eval() forward moved the biases"
    assert torch.equal(out2, out) and out2.grad_fn is None
    with pytest.raises(RuntimeError):
        out2.sum().backward()
    xg = x.cuda().requires_grad_(True)
    out3 = m(xg)  # eval() with grad mode on: differentiable, and still no update
    out3.float().square().mean().backward()
    assert torch.equal(out3, out) and torch.equal(xg.grad, dx) and torch.equal(m.biases, before)
    m.train()
    with torch.no_grad():
        m(x.cuda())
    assert torch.equal(m.biases.cpu(), LO.bias_update(before.cpu(), t[pre + "counts"].long(), LO.RATE)), "a training forward without grad mode updates too"
    assert not bad, "\n".join(bad)


def test_segmented_and_per_expert_paths_give_the_same_bits(fixture, switch):
    t = fixture
    res = {}
    for on in (True, False):
        switch(on)
        res[on] = _step(_layer("A", t), t["A.in.x"])
    assert torch.equal(res[True][0], res[False][0]), "out"
    assert torch.equal(res[True][1], res[False][1]), "dx"
    for n, g in res[True][2].items():
        assert g is not None and res[False][2][n] is not None and torch.equal(g, res[False][2][n]), n


@pytest.mark.parametrize("segmented", [True, False], ids=["segmented", "per-expert"])
def test_a_routing_that_leaves_experts_empty(segmented, switch):
    from llm_quest_amd.moe.nvidia_latent_moe import LatentMoE

    switch(segmented)
    used, T = (2, 5, 9), 70
    torch.manual_seed(40)
    m = LatentMoE(dict(LO.FIXTURE_CFG, num_experts=12, top_k=3)).cuda().train()
    assert (m.num_experts, m.top_k) == (12, 3) and m.biases.dtype == F32
    m._forced_topk = torch.stack([torch.tensor(used).roll(i % 3) for i in range(T)]).to(I32).cuda()
    x = torch.randn(2, 35, 64, generator=torch.Generator().manual_seed(41)).to(BF16)
    out, dx, grads = _step(m, x)
    assert m._routed[1].tolist() == [T if e in used else 0 for e in range(12)]
    once = {n: g.clone() for n, g in grads.items()}
    for n, g in once.items():
        assert g is not None and bool(torch.isfinite(g.float()).all()), n
        if n.startswith("routed_experts."):
            if int(n.split(".")[1]) in used:
                assert float(g.float().abs().max()) > 0, n
            else:
                assert bool((g == 0).all()), f"{n}: an expert without a token must have an exactly zero gradient"
    out2, dx2, twice = _step(m, x)  # no zero_grad in between: the second backward accumulates
    assert torch.equal(out2, out) and torch.equal(dx2, dx)
    for n, g in twice.items():
        if float(once[n].float().abs().max()) == 0.0:
            assert bool((g == 0).all()), n
        else:
            # bf16(s + bf16(s)) against 2 bf16(s), s the fp32 sum: |s - bf16(s)| <= 2^-8 |s| (bf16's unit roundoff) and one more rounding of about 2 s,
            # so at most 1.5 * 2^-8 relative per element, hence in the L2 norm
            assert LO.rel_l2(g, once[n].double() * 2) <= 1.5 * 2.0 ** -8, n


# ----------------------------------------------------------------------------------------------------------------- the activation argument
def test_existing_layers_do_not_change_with_the_activation_argument(monkeypatch):
    """``Qwen3MoE`` and ``DeepSeekMoE`` with ``activation="swiglu"`` passed explicitly to ``run_experts_forward`` / ``run_experts_backward`` give the
    bits they give without the argument."""
    import test_deepseek_moe_gpu as TD
    from llm_quest_amd import ops_moe
    from llm_quest_amd.moe.deepseek_moe import DeepSeekMoE
    from llm_quest_amd.moe.qwen3_moe import Qwen3MoE

    def qwen():
        torch.manual_seed(28)
        moe = Qwen3MoE(dict(emb_dim=64, moe_hidden_dim=64, num_experts=8, top_k=2, aux_loss_coef=0.01, dtype=BF16)).cuda().train()
        x = torch.randn(1, 70, 64, generator=torch.Generator().manual_seed(21)).to(BF16).cuda().requires_grad_(True)
        out = moe(x)
        torch.autograd.backward([out, moe.moe_loss], [torch.ones_like(out), torch.ones((), dtype=BF16, device="cuda")])
        return [out.detach(), x.grad] + [p.grad for p in moe.parameters()]

    def deepseek():
        cfg, T = TD._layer_cfg("7 routed + 1 shared, k 3, T 70")
        torch.manual_seed(8)
        moe = DeepSeekMoE(cfg).to(BF16).cuda().train()
        x = torch.randn(1, T, 64, generator=torch.Generator().manual_seed(9)).to(BF16).cuda().requires_grad_(True)
        out = moe(x)
        out.backward(torch.randn(1, T, 64, generator=torch.Generator().manual_seed(10)).to(BF16).cuda())
        return [out.detach(), x.grad] + [p.grad for p in moe.parameters()]

    plain = {"Qwen3MoE": qwen(), "DeepSeekMoE": deepseek()}
    fwd, bwd, calls = ops_moe.run_experts_forward, ops_moe.run_experts_backward, []
    monkeypatch.setattr(ops_moe, "run_experts_forward", lambda *a: (calls.append("f"), fwd(*a, activation="swiglu"))[1])
    monkeypatch.setattr(ops_moe, "run_experts_backward", lambda *a: (calls.append("b"), bwd(*a, activation="swiglu"))[1])
    explicit = {"Qwen3MoE": qwen(), "DeepSeekMoE": deepseek()}
    assert calls == ["f", "b", "f", "b"]
    for name in plain:
        assert len(plain[name]) == len(explicit[name])
        for i, (a, b) in enumerate(zip(plain[name], explicit[name])):
            assert a is not None and torch.equal(a, b), (name, i)
