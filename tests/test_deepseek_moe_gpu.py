"""DeepSeekMoE kernels (csrc/deepseek_moe.hip), the layer, the DeepSeek-V3 block that holds it and the model on the GPU, against the plain-torch
restatement (tests/deepseek_moe_oracle.py) and the reference fixture (tests/golden/deepseek_moe_tiny*).

Tolerance: the project's 1.5x rule and nothing else -- the relative L2 distance of a kernel output to the fp64 restatement is
at most 1.5 x the distance of the reference-dtype-flow restatement to the same fp64 result, with 2e-3 absolute slack only where that floor is below
1e-2.  Where the fp64 result is identically zero the kernel is held to 1e-6 absolute per element.  Integer outputs and the bias update are compared
exactly.  Where a selection enters a comparison, the restatement is evaluated on the selection the kernels made (or both on a forced one); that the
kernels select what the reference selects is checked separately, on the tokens whose selection survives a one-ulp move of the logits.
"""

import json
import os

import pytest
import torch

import deepseek_moe_oracle as MO

pytestmark = pytest.mark.gpu
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
ROUTE_CASES = [(1, 1, 1), (3, 3, 5), (7, 3, 70), (8, 2, 33), (65, 8, 64), (127, 8, 130), (128, 8, 96)]  # (E, k, T)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _kd():
    from llm_quest_amd import kernels_dsmoe as KD

    return KD


def judge(name, mine, ref_flow, exact, report):
    mine, ref_flow, exact = mine.detach().cpu(), ref_flow.detach().cpu(), exact.detach().cpu()
    assert mine.shape == exact.shape, (name, mine.shape, exact.shape)
    if float(exact.double().norm()) == 0.0:
        worst = float(mine.double().abs().max())
        print(f"  {name}: exact value is zero; kernel max |x| {worst:.3e}")
        if not worst <= 1e-6:
            report.append(f"{name}: exact value is zero, kernel max |x| {worst:.3e} > 1e-6")
        return
    floor = MO.rel_l2(ref_flow, exact)
    got = MO.rel_l2(mine, exact)
    bound = 1.5 * floor + (0.0 if floor >= 1e-2 else 2e-3)
    print(f"  {name}: kernel {got:.3e}  reference flow {floor:.3e}  bound {bound:.3e}")
    if not got <= bound:
        report.append(f"{name}: {got:.3e} > {bound:.3e} (floor {floor:.3e})")


# ----------------------------------------------------------------------------------------------------------------- router
_ROUTE = {}


def _route_bias(E, k, T, kind):
    if kind == "zero":
        return torch.zeros(E, dtype=BF16)
    probe = torch.nn.functional.softmax(MO.logits_without_boundary_tie(T, E, k, torch.zeros(E, dtype=BF16), seed=4000 + E + k + T), dim=-1)
    if kind == "lift":  # lifts the least probable expert into every selection: a probability is at most 1
        b = torch.zeros(E, dtype=BF16)
        b[int(probe.float().mean(dim=0).argmin())] = 2.0
        return b
    g = torch.Generator().manual_seed(9 + E)  # fp32 values that bf16 cannot hold, of the size of the gaps between the probabilities
    return (0.05 * torch.randn(E, generator=g)).float() + 1e-4


def route_case(E, k, T, kind):
    """bf16 logits without a boundary tie in the biased key (the last row, when there is more than one, all equal), an upstream gradient and both
    flows of the restatement; computed once per case and shared (never modified) by the tests."""
    key = (E, k, T, kind)
    if key not in _ROUTE:
        b = _route_bias(E, k, T, kind)
        x = MO.logits_without_boundary_tie(T, E, k, b, seed=4000 + E + k + T)
        if T > 1:
            x[-1] = 0.5
        dw = torch.randn(T, k, generator=torch.Generator().manual_seed(77 + T))
        c = {"x": x, "b": b, "dw": dw}
        p, idx, w, s = MO.route(x, b, k)
        c[None] = dict(p=p, idx=idx, w=w, s=s, dlogits=MO.route_bwd(x, b, k, dw.to(BF16), idx=idx))
        p64, _, w64, s64 = MO.route(x, b, k, dtype=torch.float64, idx=idx)
        c[torch.float64] = dict(p=p64, w=w64, s=s64, dlogits=MO.route_bwd(x, b, k, dw, dtype=torch.float64, idx=idx))
        _ROUTE[key] = c
    return _ROUTE[key]


@pytest.mark.parametrize("kind", ["zero", "lift", "f32"])
@pytest.mark.parametrize("E,k,T", ROUTE_CASES)
def test_route_forward_and_backward_against_the_restatement(E, k, T, kind):
    from llm_quest_amd import kernels_moe as KM

    KD = _kd()
    c = route_case(E, k, T, kind)
    x, b = c["x"].cuda(), c["b"].cuda()
    assert b.dtype == (F32 if kind == "f32" else BF16)
    p, idx, w, s = KD.route_fwd(x, b, k)
    assert torch.equal(idx.cpu().long(), c[None]["idx"]), "the selected experts differ from the restatement's"
    if kind == "zero":  # the plain top-k of p
        assert torch.equal(idx.cpu().long(), MO.topk_lowest_index_first(c[None]["p"], k)[1])
        if T > 1:
            assert idx[-1].tolist() == list(range(k))  # all keys equal: the lower expert index wins
    if kind == "lift":
        lifted = int(c["b"].float().argmax())
        assert bool((idx == lifted).any(dim=1).all()) and bool((idx[:, 0] == lifted).all())
    if E == 3:
        assert bool((idx.sort(dim=1).values.cpu() == torch.arange(3)).all())  # every expert selected
    assert bool((idx.sort(dim=1).values[:, 1:] != idx.sort(dim=1).values[:, :-1]).all()) if k > 1 else True
    bad = []
    for name, mine in (("p", p), ("w", w), ("s", s)):
        judge(name, mine, c[None][name], c[torch.float64][name], bad)
    v = p.float().gather(1, idx.long())  # the kernel's rounding points: the UNBIASED probabilities, s a bf16 value, w = bf16(v / s)
    assert torch.equal(s, s.to(BF16).float()) and torch.equal(w, (v / s.unsqueeze(1)).to(BF16))
    dl = KM.route_bwd(c["dw"].cuda(), w, s, idx, p)
    judge("dlogits", dl, c[None]["dlogits"], c[torch.float64]["dlogits"], bad)
    # a column slice of a wider buffer whose pad columns hold large values routes the same, forward and backward
    wide = torch.full((T, E + 25), 60.0, dtype=BF16, device="cuda")
    wide[:, 8 : 8 + E] = x
    p3, idx3, w3, s3 = KD.route_fwd(wide[:, 8 : 8 + E], b, k)
    assert torch.equal(p3, p) and torch.equal(idx3, idx) and torch.equal(w3, w) and torch.equal(s3, s)
    dwide = torch.full((T, E + 25), 9.0, dtype=BF16, device="cuda")
    KM.route_bwd(c["dw"].cuda(), w, s, idx, p, dlogits=dwide[:, 8 : 8 + E])
    assert torch.equal(dwide[:, 8 : 8 + E], dl) and bool((dwide[:, :8] == 9.0).all()) and bool((dwide[:, 8 + E :] == 9.0).all())
    # forced selection: the given experts, weighed with this call's own probabilities
    forced = ((idx.long() + 1) % E).flip(1).to(I32).contiguous() if E > k else idx.flip(1).contiguous()
    pf, idxf, wf, sf = KD.route_fwd(x, b, k, forced_idx=forced)
    _, _, wr, sr = MO.route(c["x"], c["b"], k, idx=forced.cpu().long())
    assert torch.equal(idxf, forced) and torch.equal(pf, p)
    vf = pf.float().gather(1, forced.long())
    acc = torch.zeros(T, device="cuda")  # s: the sum in slot order
    for j in range(k):
        acc = acc + vf[:, j]
    assert torch.equal(sf, acc.to(BF16).float()) and torch.equal(wf, (vf / sf.unsqueeze(1)).to(BF16))
    _, _, w64, s64 = MO.route(c["x"], c["b"], k, dtype=torch.float64, idx=forced.cpu().long())
    judge("forced w", wf, wr, w64, bad)
    judge("forced s", sf, sr, s64, bad)
    assert not bad, "\n".join(bad)


# ----------------------------------------------------------------------------------------------------------------- bias update
def _update_cases():
    g = torch.Generator().manual_seed(5)
    return {
        "E=7 above, below, at the mean, one empty": torch.tensor([5, 1, 3, 3, 0, 6, 3]),
        "E=1": torch.tensor([9]),
        "E=128": torch.randint(0, 50, (128,), generator=g),
        "E=7 all equal": torch.full((7,), 4),
    }


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("name", list(_update_cases()))
def test_bias_update_and_max_violation(name, dtype):
    KD = _kd()
    counts = _update_cases()[name]
    E = counts.numel()
    g = torch.Generator().manual_seed(E)
    b0 = (0.05 * torch.randn(E, generator=g)).to(dtype)
    if dtype == BF16:
        b0[0] = 4.0  # a bf16 ulp of 2^-5: the increment of 1e-3 is lost to rounding
    rate = 1e-3
    want = MO.bias_update(b0, counts, rate)
    b = b0.clone().cuda()
    mv = KD.bias_update(counts.to(I32).cuda(), b, rate)
    assert b.dtype == dtype and torch.equal(b.cpu(), want), (b.cpu(), want)
    if dtype == BF16:
        assert float(b[0]) == 4.0
    at_mean = counts.float() == counts.float().mean()
    assert torch.equal(b.cpu()[at_mean], b0[at_mean])  # sign 0: unchanged
    bad = []
    judge("max_vio", mv.reshape(()), MO.max_violation(counts), MO.max_violation(counts, torch.float64), bad)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("T,N,pad", [(1, 8, 0), (33, 40, 8), (130, 96, 0), (4100, 520, 24)])
def test_fixed_order_column_sums(T, N, pad):
    """The bias gradients' column sums: against fp64 within fp32 summation error, the same bits in two runs, row-strided views."""
    KD = _kd()
    g = torch.Generator().manual_seed(T + N)
    wide = torch.randn(T, N + pad, generator=g).to(BF16).cuda()
    x = wide[:, pad : pad + N] if pad else wide
    a, b = KD.colsum(x), KD.colsum(x)
    assert a.dtype == F32 and tuple(a.shape) == (N,) and torch.equal(a, b)
    exact = x.double().sum(dim=0)
    scale = x.double().abs().sum(dim=0)
    # fp32 sums: every term passes fewer than 64 additions (rows of a wave, the four waves, the fold of at most 128 parts), each within 2^-24 relative
    assert bool(((a.double() - exact).abs() <= 2.0 ** -18 * scale + 1e-30).all())


# ----------------------------------------------------------------------------------------------------------------- shared experts
def _load(module, sd):
    missing, unexpected = module.load_state_dict(sd, strict=False)
    assert not unexpected and set(missing) <= {"mask", "cos", "sin"}, (missing, unexpected)
    return module


def _grads_of(module):
    return {n: (p.grad if p.grad is not None else None) for n, p in module.named_parameters()}


@pytest.mark.parametrize("T", [1, 33, 130])
@pytest.mark.parametrize("hidden", [8, 40])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_shared_experts_against_the_restatement(n, hidden, T):
    from llm_quest_amd.moe.deepseek_moe import VectorizedSharedExperts

    d = 64
    cfg = dict(emb_dim=d, hidden_dim=hidden, dtype=BF16)
    g = torch.Generator().manual_seed(100 * n + hidden + T)
    r = lambda *shape, scale: (scale * torch.randn(*shape, generator=g)).to(BF16)
    sd = {"lin1.weight": r(n, d, hidden, scale=d ** -0.5), "lin1.bias": r(n, hidden, scale=0.3), "lin2.weight": r(n, hidden, d, scale=hidden ** -0.5),
          "lin2.bias": r(n, d, scale=0.3)}
    x, dy = r(T, d, scale=1.0), r(T, d, scale=1.0)
    sh = _load(VectorizedSharedExperts(n, cfg, 1).to(BF16), sd).cuda()
    xg = x.view(1, T, d).cuda().requires_grad_(True)
    y = sh(xg)
    y.backward(dy.view(1, T, d).cuda())
    ops = [sd[k] for k in ("lin1.weight", "lin1.bias", "lin2.weight", "lin2.bias")]
    ref, exact = MO.shared_grads(x, *ops, dy), MO.shared_grads(x, *ops, dy, dtype=torch.float64)
    mine = (y.view(T, d), xg.grad.view(T, d), sh.lin1.weight.grad, sh.lin1.bias.grad, sh.lin2.weight.grad, sh.lin2.bias.grad)
    bad = []
    for name, m_, r_, e_ in zip(("out", "dx", "d lin1.weight", "d lin1.bias", "d lin2.weight", "d lin2.bias"), mine, ref, exact):
        judge(name, m_, r_, e_, bad)
    with torch.no_grad():
        assert torch.equal(sh(xg), y)
    assert not bad, "\n".join(bad)


# ----------------------------------------------------------------------------------------------------------------- layer
LAYER_CASES = {
    "7 routed + 1 shared, k 3, T 1": (dict(num_experts=8, num_shared_experts=1, top_k=3, moe_scaling_factor="auto", hidden_dim=128), 1),
    "7 routed + 1 shared, k 3, T 70": (dict(num_experts=8, num_shared_experts=1, top_k=3, moe_scaling_factor="auto", hidden_dim=128), 70),
    "7 routed + 1 shared, k 3, T 130": (dict(num_experts=8, num_shared_experts=1, top_k=3, moe_scaling_factor="auto", hidden_dim=128), 130),
    "8 routed, no shared, k 2": (dict(num_experts=8, num_shared_experts=0, top_k=2, moe_scaling_factor="auto", hidden_dim=64), 70),
    "16 routed + 2 shared, k 4, factor 1": (dict(num_experts=18, num_shared_experts=2, top_k=4, moe_scaling_factor=1, hidden_dim=32), 70),
}
_LAYER = {}


def _layer_cfg(name):
    over, T = LAYER_CASES[name]
    return dict(emb_dim=64, dtype=BF16, moe_bias_update_rate=1e-3, **over), T


def _layer_run(name):
    """One forward + backward of the layer with normal routing, and both flows of the restatement on the selection the kernels made."""
    if name in _LAYER:
        return _LAYER[name]
    from llm_quest_amd.moe.deepseek_moe import DeepSeekMoE

    cfg, T = _layer_cfg(name)
    E = cfg["num_experts"] - cfg["num_shared_experts"]
    b0 = torch.zeros(E)
    b0[1], b0[E - 2] = -2.0, -2.0  # two experts that no token selects (k <= E - 2 in every case)
    b0[0] = 0.0625
    sd = MO.layer_state(cfg, seed=31 + E, biases=b0)
    g = torch.Generator().manual_seed(7 + T)
    x, dy = torch.randn(T, 64, generator=g).to(BF16), torch.randn(T, 64, generator=g).to(BF16)

    def run():
        moe = _load(DeepSeekMoE(cfg).to(BF16), sd).cuda().train()
        assert moe.biases.dtype == BF16 and "biases" not in dict(moe.named_parameters())
        xg = x.view(1, T, 64).cuda().requires_grad_(True)
        y = moe(xg)
        y.backward(dy.view(1, T, 64).cuda())
        return moe, y.detach().view(T, 64), xg.grad.view(T, 64)

    moe, y, dx = run()
    idx, counts = [t.cpu().long() for t in moe._routed]
    rec = {}
    MO.moe_layer(sd, "", x, cfg, record=rec)  # the reference flow's own selection
    ref = MO.layer_grads(sd, "", x, cfg, dy, idx=idx)
    exact = MO.layer_grads(sd, "", x, cfg, dy, dtype=torch.float64, idx=idx)
    _LAYER[name] = dict(cfg=cfg, T=T, E=E, sd=sd, x=x, dy=dy, moe=moe, y=y, dx=dx, idx=idx, counts=counts, rec=rec, ref=ref, exact=exact, run=run, b0=b0)
    return _LAYER[name]


@pytest.mark.parametrize("name", list(LAYER_CASES))
def test_layer_against_the_restatement(name):
    c = _layer_run(name)
    moe, E, k = c["moe"], c["E"], c["cfg"]["top_k"]
    idx, counts = c["idx"], c["counts"]
    assert torch.equal(counts, MO.counts_of(idx, E)) and int(counts[1]) == 0 and int(counts[E - 2]) == 0
    robust = MO.robust_tokens(c["rec"]["logits"], c["b0"].to(BF16), k)
    same = (idx.sort(dim=1).values == c["rec"]["idx"].sort(dim=1).values).all(dim=1)
    print(f"  {int(robust.sum())} of {robust.numel()} tokens robust; the selection agrees on {int(same.sum())}")
    assert bool(same[robust].all()), "a robust token selects other experts than the restatement"
    assert torch.equal(moe.biases.cpu(), MO.bias_update(c["b0"].to(BF16), counts, 1e-3))
    bad = []
    judge("max_vio", moe.max_vio, MO.max_violation(counts), MO.max_violation(counts, torch.float64), bad)
    assert moe.max_vio.dim() == 0
    judge("out", c["y"], c["ref"][0], c["exact"][0], bad)
    judge("dx", c["dx"], c["ref"][1], c["exact"][1], bad)
    grads = _grads_of(moe)
    assert set(grads) == set(c["ref"][2])
    for n, g in grads.items():
        assert g is not None, n
        judge("d " + n, g, c["ref"][2][n], c["exact"][2][n], bad)
        if n.startswith("routed_experts."):
            e = int(n.split(".")[1])
            if int(counts[e]) == 0:
                assert bool((g == 0).all()), f"{n}: an expert without a token must have an exactly zero gradient"
    assert not bad, "\n".join(bad)


def test_layer_two_runs_are_bit_identical():
    c = _layer_run("7 routed + 1 shared, k 3, T 130")
    moe2, y2, dx2 = c["run"]()
    assert torch.equal(y2, c["y"]) and torch.equal(dx2, c["dx"]) and torch.equal(moe2.biases, c["moe"].biases)
    assert torch.equal(moe2._routed[0], c["moe"]._routed[0])
    g1, g2 = _grads_of(c["moe"]), _grads_of(moe2)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n


def test_every_forward_updates_the_biases_grad_or_not():
    from llm_quest_amd.moe.deepseek_moe import DeepSeekMoE

    cfg, T = _layer_cfg("7 routed + 1 shared, k 3, T 70")
    sd = MO.layer_state(cfg, seed=3)
    moe = _load(DeepSeekMoE(cfg).to(BF16), sd).cuda().train()
    x = torch.randn(1, T, 64, generator=torch.Generator().manual_seed(1)).to(BF16).cuda()
    forced = torch.stack([torch.tensor([0, 2, 5]) if t % 3 else torch.tensor([2, 5, 6]) for t in range(T)]).to(I32).cuda()
    moe._forced_topk = forced
    counts = MO.counts_of(forced.cpu().long(), 7)
    b = sd["biases"].clone()
    moe(x)
    b = MO.bias_update(b, counts, 1e-3)
    assert torch.equal(moe.biases.cpu(), b) and torch.equal(moe._routed[0], forced)
    moe.eval()
    with torch.no_grad():
        moe(x)
    b = MO.bias_update(b, counts, 1e-3)
    assert torch.equal(moe.biases.cpu(), b), "an eval() / no_grad() forward applies the update too"
    moe._forced_topk = None
    moe.biases = moe.biases.float()  # an fp32 buffer works too: an fp32 key, an fp32 update
    before = moe.biases.clone()
    with torch.no_grad():
        moe(x)
    c2 = moe._routed[1].cpu().long()
    assert moe.biases.dtype == F32 and torch.equal(moe.biases.cpu(), MO.bias_update(before.cpu(), c2, 1e-3))


# ----------------------------------------------------------------------------------------------------------------- model on the fixture
@pytest.fixture(scope="module")
def fixture():
    return MO.load_fixture("deepseek_moe_tiny")


CFG = MO.TINY_DEEPSEEK_MOE
LAYERS = MO.moe_layers(CFG)


def _model(t):
    from llm_quest_amd.llama3_to_deepseekv3.deepseek_model import DeepSeekV3Model

    torch.manual_seed(0)
    m = _load(DeepSeekV3Model(dict(CFG)).to(BF16), {k[3:]: v for k, v in t.items() if k.startswith("sd.")})
    return m.cuda().train()


def _inputs(t, dev="cuda"):
    depth = CFG["mtp_depth"]
    return (t["in.ids"].to(dev), t["in.targets"].to(dev), [t[f"in.shifted_x.{k}"].to(dev) for k in range(depth)],
            [t[f"in.shifted_y.{k}"].to(dev) for k in range(depth)])


def test_model_on_the_fixture_with_the_selection_forced(fixture):
    t = fixture
    m = _model(t)
    for i in LAYERS:
        m.main_model.trf_blocks[i].ffn._forced_topk = t[f"moe.{i}.topk_idxs"].cuda()
    ids, tgt, sx, sy = _inputs(t)
    loss = m(ids, tgt, sx, sy)
    loss.backward()
    bad = []
    for i in LAYERS:
        ffn, pre = m.main_model.trf_blocks[i].ffn, f"moe.{i}."
        assert torch.equal(ffn._routed[0].cpu(), t[pre + "topk_idxs"]) and torch.equal(ffn._routed[1].cpu(), t[pre + "counts"]), i
        assert torch.equal(ffn.biases.cpu(), t[pre + "biases"]), f"layer {i}: updated biases"
        judge(pre + "max_vio", ffn.max_vio.reshape(1), t[pre + "max_vio"], MO.max_violation(t[pre + "counts"].long(), torch.float64).reshape(1), bad)
    judge("loss", loss.reshape(1), t["out.loss"].reshape(1), t["twin.loss"].reshape(1), bad)
    with open(os.path.join(MO.GOLDEN, "deepseek_moe_signatures.json")) as f:
        floors = json.load(f)["floors"]
    judged = 0
    for name, p in m.named_parameters():
        if name.startswith("mtp_modules.") and (".emb_layer." in name or ".out_layer." in name):
            continue
        if p.grad is None:  # the last MTP module's block feeds nothing (its logits come from the down-projected input): no gradient, as upstream
            assert name.startswith("mtp_modules.") and ".trf_block." in name and "grad." + name not in t, name
            continue
        if "grad." + name not in t:  # an expert that received no token: the reference leaves None, here an exactly zero gradient
            assert ".routed_experts." in name and bool((p.grad == 0).all()), name
            continue
        floor = MO.rel_l2(t["grad." + name], t["twin.grad." + name])
        assert abs(floor - floors[name]) <= 1e-3 * max(floor, 1e-30) + 1e-12, name
        if floor <= 0.1:
            judge("d " + name, p.grad, t["grad." + name], t["twin.grad." + name], bad)
            judged += 1
    want = sum(1 for v in floors.values() if v <= 0.1)
    print(f"  {judged} gradients judged of {len(floors)}")
    assert judged == want and judged >= 0.9 * len(floors)
    for blk in m.main_model.trf_blocks:
        lo, hi = blk._arena.grad.data_ptr(), blk._arena.grad.data_ptr() + blk._arena.grad.numel() * 2
        for name, p in blk.named_parameters():
            assert lo <= p.grad.data_ptr() < hi, name
    m.eval()
    with torch.no_grad():
        logits = m(ids, None, None, None)
    judge("logits", logits, t["out.logits"], t["twin.logits"], bad)
    assert not bad, "\n".join(bad)


def test_model_on_the_fixture_with_normal_routing(fixture):
    """Only the first MoE layer is judged against the fixture's selection: a deeper layer's input already carries the rounding differences of the
    layers before it, so its logits are no longer the reference's to within one ulp."""
    t = fixture
    m = _model(t)
    ids, tgt, sx, sy = _inputs(t)
    loss = m(ids, tgt, sx, sy)
    loss.backward()
    assert bool(torch.isfinite(loss))
    for name, p in m.named_parameters():
        if p.grad is None:  # the last MTP module's block, as upstream
            assert name.startswith("mtp_modules.") and ".trf_block." in name, name
            continue
        assert bool(torch.isfinite(p.grad).all()), name
    first =m.main_model.trf_blocks[LAYERS[0]].ffn
    assert float(first.gate.weight.grad.float().abs().max()) > 0 and float(first.gate.bias.grad.float().abs().max()) > 0
    pre = f"moe.{LAYERS[0]}."
    robust = t[pre + "robust"].bool()
    mine, ref = first._routed[0].cpu().long().sort(dim=1).values, t[pre + "topk_idxs"].long().sort(dim=1).values
    same = (mine == ref).all(dim=1)
    print(f"  first MoE layer: {int(robust.sum())} of {robust.numel()} tokens robust; the selection agrees on {int(same.sum())}")
    assert int(robust.sum()) * 10 >= 9 * robust.numel() and bool(same[robust].all())
    for i in LAYERS:
        assert bool(torch.isfinite(m.main_model.trf_blocks[i].ffn.max_vio))


def test_twenty_optimizer_steps_lower_the_loss(fixture):
    from llm_quest_amd.moe.deepseek_moe import max_violation_step
    from llm_quest_amd.optim import ArenaAdamW

    t = fixture
    m = _model(t)
    assert not any(n.endswith("biases") for n, _ in m.named_parameters())
    ids, tgt, sx, sy = _inputs(t)
    opt = ArenaAdamW(m.parameters(), lr=1e-3, weight_decay=0.0).attach(m)
    ffns = [m.main_model.trf_blocks[i].ffn for i in LAYERS]
    losses = []
    for step in range(21):
        before = [f.biases.clone() for f in ffns]
        loss = m(ids, tgt, sx, sy)
        losses.append(loss.detach())
        for f, b in zip(ffns, before):  # biases move by the update rule ...
            assert torch.equal(f.biases.cpu(), MO.bias_update(b.cpu(), f._routed[1].cpu().long(), CFG["moe_bias_update_rate"]))
        if step == 20:
            break
        opt.zero_grad(set_to_none=True)
        loss.backward()
        after = [f.biases.clone() for f in ffns]
        opt.step()
        for f, b in zip(ffns, after):  # ... and by nothing else
            assert torch.equal(f.biases, b)
    mv = max_violation_step(m)
    assert mv.dim() == 0 and abs(float(mv) - sum(float(f.max_vio) for f in ffns) / len(ffns)) < 1e-6
    first, last = float(losses[0]), float(losses[-1])
    print(f"  loss at step 0: {first:.4f}, at step 20: {last:.4f}")
    assert last == last and last < first
