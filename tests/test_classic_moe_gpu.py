"""Classic-MoE kernels (csrc/classic_moe.hip), ``ExpertGeLU`` on its own and the layer on the GPU, against the plain-torch restatement
(tests/classic_moe_oracle.py) and the reference fixture (tests/golden/classic_moe_tiny*).

Tolerance: the project's 1.5x rule through ``test_deepseek_moe_gpu.judge`` and nothing else -- the relative L2 distance of a
kernel output to the fp64 restatement is at most 1.5 x the distance of the reference-dtype-flow restatement to the same fp64 result, with 2e-3 absolute
slack only where that floor is below 1e-2; where the fp64 result is identically zero the kernel is held to 1e-6 absolute per element.  Integer outputs
(idx, counts) and the kernels' own rounding points are compared exactly.  The router's inputs have no boundary tie, and the layer tests force the
fixture's selection.
"""

import pytest
import torch

import classic_moe_oracle as CO
from test_classic_moe_cpu import refusal_checks
from test_deepseek_moe_gpu import judge

pytestmark = pytest.mark.gpu
BF16, F32, I32, F64 = torch.bfloat16, torch.float32, torch.int32, torch.float64
ROUTE_CASES = [(1, 1, 1), (3, 3, 5), (8, 2, 70), (16, 8, 33), (127, 8, 130), (128, 8, 96)]  # (E, k, T)
ACT_CASES = [(1, 8), (33, 40), (130, 96), (515, 520)]  # (R, N)
ALIGN = 32  # mi355_moe_row_align(), asserted below
SENT = 7.0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


@pytest.fixture
def switch(monkeypatch):
    """Sets ``ops_moe.SEGMENTED`` for one test (the layers read it there, at call time)."""
    from llm_quest_amd import ops_moe

    return lambda on: monkeypatch.setattr(ops_moe, "SEGMENTED", bool(on))


def _kc():
    from llm_quest_amd import kernels_cmoe as KC

    return KC


# ----------------------------------------------------------------------------------------------------------------- router
_ROUTE = {}
G_LOSS, LOAD, ZC = 3.0, 10e-2, 1e-3


def route_case(E, k, T, extreme=False):
    """bf16 logits without a boundary tie, an upstream gradient and both flows of the restatement, with and without the loss's gradient; computed once
    per case and shared (never modified) by the tests.  ``extreme``: the first rows hold logits of +-120."""
    key = (E, k, T, extreme)
    if key not in _ROUTE:
        x = CO.tie_free_logits(T, E, k, seed=5000 + E + k + T)
        if extreme:
            assert E == 8 and k == 2
            x[0] = torch.tensor([120.0, 118.0, 116.0, -120.0, -120.0, -118.0, 100.0, -100.0]).to(BF16)
            x[1] = torch.tensor([-120.0, -118.0, -116.0, -114.0, -120.0, -120.0, -120.0, -120.0]).to(BF16)
            x[2] = torch.tensor([-120.0, 120.0, 117.0, 0.0, 1.0, -1.0, 114.0, 60.0]).to(BF16)
            assert not bool(CO.boundary_tie(torch.softmax(x, dim=-1), k).any())
        dw = torch.randn(T, k, generator=torch.Generator().manual_seed(77 + T))
        p, idx, w, s, lse = CO.route(x, k)
        p64, _, w64, s64, lse64 = CO.route(x, k, dtype=F64, idx=idx)
        c = dict(x=x, dw=dw, idx=idx, ref=dict(p=p, w=w, s=s, lse=lse, loss=CO.moe_loss(p, idx, lse, LOAD, ZC)),
                 exact=dict(p=p64, w=w64, s=s64, lse=lse64, loss=CO.moe_loss(p64, idx, lse64, LOAD, ZC)))
        for g in (None, G_LOSS):
            c["ref"][g] = CO.route_bwd(x, k, dw.to(BF16), g, LOAD, ZC, idx=idx)
            c["exact"][g] = CO.route_bwd(x, k, dw, g, LOAD, ZC, dtype=F64, idx=idx)
        _ROUTE[key] = c
    return _ROUTE[key]


def _own_rounding_points(p, idx, w, s, lse):
    """w and s exactly from the kernel's own p: s = bf16(slot-order fp32 sum), w = bf16(v / s); an index that is no expert weighs 0; lse is a bf16 value."""
    E = p.shape[1]
    ok = (idx >= 0) & (idx < E)
    v = torch.where(ok, p.float().gather(1, idx.long().clamp(0, E - 1)), torch.zeros((), device=p.device))
    acc = torch.zeros(p.shape[0], device=p.device)
    for j in range(idx.shape[1]):
        acc = acc + v[:, j]
    assert torch.equal(s, acc.to(BF16).float()), "s is not bf16(the slot-order sum of the selected probabilities)"
    assert torch.equal(w, (v / s.unsqueeze(1)).to(BF16)), "w is not bf16(v / s)"
    assert torch.equal(lse, lse.to(BF16).float()), "lse is not a bf16 value"


def _loss_of(KC, KM, p, idx, lse, E):
    from llm_quest_amd import kernels_dsmoe as KD

    Ep = (E + 7) // 8 * 8
    pb = torch.zeros((p.shape[0], Ep), dtype=BF16, device="cuda")
    pb[:, :E] = p
    counts, _, _, _, load = KM.plan(idx, E, KD.colsum(pb)[:E], LOAD)
    return counts, KC.loss(lse, ZC, load), KC.loss(lse, ZC)


@pytest.mark.parametrize("E,k,T,extreme", [c + (False,) for c in ROUTE_CASES] + [(8, 2, 70, True)])
def test_route_forward_backward_and_loss_against_the_restatement(E, k, T, extreme):
    from llm_quest_amd import kernels_moe as KM

    KC = _kc()
    c = route_case(E, k, T, extreme)
    x, dw = c["x"].cuda(), c["dw"].cuda()
    bad = []
    p, idx, w, s, lse = KC.route_fwd(x, k)
    assert torch.equal(idx.cpu().long(), c["idx"]), "the selected experts differ from the restatement's"
    p0, idx0, w0, s0 = KM.route_fwd(x, k)  # exactly what mi355_moe_route_fwd writes
    assert torch.equal(p, p0) and torch.equal(idx, idx0) and torch.equal(w, w0) and torch.equal(s, s0)
    assert bool(torch.isfinite(lse).all())
    for name, mine in (("p", p), ("w", w), ("s", s), ("lse", lse)):
        judge(name, mine, c["ref"][name], c["exact"][name], bad)
    _own_rounding_points(p, idx, w, s, lse)
    counts, loss, zonly = _loss_of(KC, KM, p, idx, lse, E)
    assert torch.equal(counts.cpu().long(), CO.counts_of(c["idx"], E))
    assert loss.dtype == F32 and tuple(loss.shape) == (1,) and torch.equal(loss, loss.to(BF16).float()) and bool(torch.isfinite(loss).all())
    judge("moe_loss", loss.reshape(()), c["ref"]["loss"], c["exact"]["loss"], bad)
    q = (lse * lse).to(BF16).float()  # the z-loss alone: its roundings sit where the header says, the sum's order aside
    zm = (q.double().sum() / T).float().to(BF16).float()
    # (one bf16 step in the mean, at most 2^-7 relative, where the fp32 and the fp64 sum fall on two sides of a rounding boundary; the product's rounding can add one)
    assert abs(float(zonly) - float((ZC * zm).to(BF16))) <= 2.0 ** -6 * abs(float(zonly)), "z-loss: not bf16(z_coeff * bf16(mean(bf16(lse^2))))"
    assert torch.equal(KC.loss(lse, ZC, None), zonly), "two calls differ"
    g = torch.tensor([G_LOSS], dtype=F32, device="cuda")
    for gg, dev in ((None, None), (G_LOSS, g)):
        dl = KC.route_bwd(dw, w, s, idx, p, counts, dev, LOAD, ZC, lse)
        assert bool(torch.isfinite(dl.float()).all())
        judge(f"dlogits (g = {gg})", dl, c["ref"][gg], c["exact"][gg], bad)
        if gg is None:  # without g neither loss term: mi355_moe_route_bwd's bits, and counts / lse are not needed
            assert torch.equal(dl, KM.route_bwd(dw, w, s, idx, p)) and torch.equal(dl, KC.route_bwd(dw, w, s, idx, p))
    # a column slice of a wider buffer whose pad columns hold large values routes the same, forward and backward
    wide = torch.full((T, E + 25), 60.0, dtype=BF16, device="cuda")
    wide[:, 8 : 8 + E] = x
    r3 = KC.route_fwd(wide[:, 8 : 8 + E], k)
    assert all(torch.equal(a, b) for a, b in zip(r3, (p, idx, w, s, lse)))
    dwide = torch.full((T, E + 25), 9.0, dtype=BF16, device="cuda")
    KC.route_bwd(dw, w, s, idx, p, counts, g, LOAD, ZC, lse, dlogits=dwide[:, 8 : 8 + E])
    assert torch.equal(dwide[:, 8 : 8 + E], dl) and bool((dwide[:, :8] == 9.0).all()) and bool((dwide[:, 8 + E :] == 9.0).all())
    # forced selection: the given experts, weighed with this call's own probabilities
    forced = ((idx.long() + 1) % E).flip(1).to(I32).contiguous() if E > k else idx.flip(1).contiguous()
    pf, idxf, wf, sf, lsef = KC.route_fwd(x, k, forced_idx=forced)
    assert torch.equal(idxf, forced) and torch.equal(pf, p) and torch.equal(lsef, lse)
    fi = forced.cpu().long()
    if not extreme:  # (the extreme rows' other experts have probability 0: s = 0 there, in every flow)
        _own_rounding_points(pf, idxf, wf, sf, lsef)
        _, _, wr, sr, _ = CO.route(c["x"], k, idx=fi)
        _, _, w64, s64, _ = CO.route(c["x"], k, dtype=F64, idx=fi)
        judge("forced w", wf, wr, w64, bad)
        judge("forced s", sf, sr, s64, bad)
        countsf, lossf, _ = _loss_of(KC, KM, pf, idxf, lsef, E)
        for gg, dev in ((None, None), (G_LOSS, g)):
            dlf = KC.route_bwd(dw, wf, sf, idxf, pf, countsf, dev, LOAD, ZC, lsef)
            judge(f"forced dlogits (g = {gg})", dlf, CO.route_bwd(c["x"], k, c["dw"].to(BF16), gg, LOAD, ZC, idx=fi),
                  CO.route_bwd(c["x"], k, c["dw"], gg, LOAD, ZC, dtype=F64, idx=fi), bad)
        if E > 1 and k > 1:  # an index that is no expert weighs 0
            off = forced.clone()
            off[:, 0] = torch.where(torch.arange(T, device="cuda") % 2 == 0, E, -1).to(I32)
            po, idxo, wo, so, lseo = KC.route_fwd(x, k, forced_idx=off)
            assert torch.equal(idxo, off) and bool((wo[:, 0] == 0).all())
            _own_rounding_points(po, idxo, wo, so, lseo)
    assert not bad, "\n".join(bad)


# ----------------------------------------------------------------------------------------------------------------- bias (+ GELU) on the sorted buffer
def _tables(R):
    """Segment tables over R sorted rows, every start on the plan's alignment: an expert owning all rows beside two empty ones; and an empty expert, a
    one-row expert and (R permitting) two more behind padding rows."""
    up = lambda n: (n + ALIGN - 1) // ALIGN * ALIGN
    own_all = ([0, R, 0], [0, 0, up(R), up(R)])
    if R <= ALIGN:
        mixed = ([0, min(1, R), 0, 0], [0, 0, ALIGN, ALIGN, ALIGN])
    elif R <= 2 * ALIGN:
        mixed = ([0, 1, R - ALIGN, 0], [0, 0, ALIGN, 2 * ALIGN, 2 * ALIGN])
    else:
        n2 = (R - ALIGN) // 2 - 3
        o3 = up(ALIGN + n2)
        mixed = ([0, 1, n2, R - o3], [0, 0, ALIGN, o3, up(R)])
    return {"own_all": own_all, "mixed": mixed}


def _padded(t, rows=1, cols=8):
    """``t`` as the interior view of a buffer with sentinel guard rows and pad columns around it -> (view, buffer)."""
    R, N = t.shape
    buf = torch.full((R + 2 * rows, N + 2 * cols), SENT, dtype=t.dtype, device="cuda")
    view = buf[rows : rows + R, cols : cols + N]
    view.copy_(t)
    return view, buf


def _guards_untouched(buf, R, N, rows=1, cols=8):
    return bool((buf[:rows] == SENT).all()) and bool((buf[rows + R :] == SENT).all()) and bool((buf[:, :cols] == SENT).all()) and bool((buf[:, cols + N :] == SENT).all())


@pytest.mark.parametrize("table", ["own_all", "mixed"])
@pytest.mark.parametrize("R,N", ACT_CASES)
def test_bias_gelu_and_bias_only_forward_and_backward(R, N, table):
    from llm_quest_amd import kernels_moe as KM

    KC = _kc()
    assert KM.row_align() == ALIGN
    counts_l, offsets_l = _tables(R)[table]
    E = len(counts_l)
    counts, offsets = torch.tensor(counts_l, dtype=I32), torch.tensor(offsets_l, dtype=I32)
    e_of = CO.row_experts(counts, offsets, R)
    live = e_of >= 0
    assert int(live.sum()) == sum(counts_l) and (table == "own_all" or R == 1 or not bool(live.all())), "the mixed tables have padding rows"
    g = torch.Generator().manual_seed(R + N)
    z = torch.randn(R, N, generator=g).to(BF16)
    z[~live] = SENT  # padding rows hold a sentinel: never read into a result, never written
    bias = (0.5 * torch.randn(E, N, generator=g)).to(BF16)
    dact = torch.randn(R, N, generator=g).to(BF16)
    pre_r, act_r, dpre_r = CO.bias_act_grads(z, bias, e_of, dact)
    pre_e, act_e, dpre_e = CO.bias_act_grads(z, bias, e_of, dact, dtype=F64)
    bbuf = torch.full((E, 1, N + 8), SENT, dtype=BF16, device="cuda")  # the experts' biases at a stride, sentinels between them
    bstack = bbuf[:, :, :N]
    bstack.copy_(bias.view(E, 1, N))
    cd, od, lv = counts.cuda(), offsets.cuda(), live.cuda()

    def run(kind, separate):
        zv, zbuf = _padded(z.cuda())
        pre_v, pre_buf = _padded(torch.full((R, N), SENT, dtype=BF16)) if separate else (None, None)
        act_v, act_buf = _padded(torch.full((R, N), SENT, dtype=BF16)) if kind else (None, None)
        got = KC.bias_act_fwd(zv, bstack, cd, od, gelu=bool(kind), pre=pre_v, act=act_v)
        assert (got is act_v) if kind else got is None
        for buf in (zbuf, pre_buf, act_buf):
            assert buf is None or _guards_untouched(buf, R, N), "a guard row or a pad column was written"
        dst = pre_v if separate else zv
        for v in (dst, act_v):
            assert v is None or bool((v[~lv] == SENT).all()), "a padding row was written"
        if separate:
            assert torch.equal(zv.cpu(), z), "z must stay as it was when pre has its own destination"
        assert bool((bbuf[:, :, N:] == SENT).all())
        return dst.contiguous(), None if act_v is None else act_v.contiguous()

    bad = []
    pre, act = run(1, False)
    want = (z.cuda().float() + bstack.view(E, N)[e_of.clamp_min(0).cuda()].float()).to(BF16)
    assert torch.equal(pre[lv], want[lv]), "pre is not bf16(z + bias[e(r)])"
    pre2, act2 = run(1, True)
    assert torch.equal(pre2[lv], pre[lv]) and torch.equal(act2[lv], act[lv]), "in place and with a destination differ"
    pre3, act3 = run(1, False)
    assert torch.equal(pre3, pre) and torch.equal(act3, act), "two runs differ"
    y0, none = run(0, False)
    assert none is None and torch.equal(y0[lv], pre[lv]), "bias only: the same sum"
    assert torch.equal(run(0, True)[0][lv], pre[lv])
    judge("pre", pre[lv], pre_r[live], pre_e[live], bad)
    judge("act", act[lv], act_r[live], act_e[live], bad)
    # the backward on the contiguous buffers: padding rows may hold anything, the live rows are judged
    dpre = KC.gelu_bwd(pre, dact.cuda())
    assert torch.equal(dpre, KC.gelu_bwd(pre, dact.cuda()))
    own = CO.bias_act_grads(pre.cpu(), torch.zeros(E, N, dtype=BF16), e_of, dact, dtype=F64)[2]  # gelu' at the kernel's own pre: no second rounding but dpre's
    assert CO.rel_l2(dpre[lv].cpu(), own[live]) <= 2.0 ** -8, "dpre is not one bf16 rounding away from dact * gelu'(pre)"
    judge("dpre", dpre[lv], dpre_r[live], dpre_e[live], bad)
    assert not bad, "\n".join(bad)


# ----------------------------------------------------------------------------------------------------------------- the biases' gradients
def _colsum_table(E):
    counts = [3000] if E == 1 else [0, 1, 3000] + [(7 * e) % 40 for e in range(3, E)]
    offsets, off = [], 0
    for c in counts:
        offsets.append(off)
        off += (c + ALIGN - 1) // ALIGN * ALIGN
    return counts, offsets + [off]


@pytest.mark.parametrize("N", [8, 40, 768])
@pytest.mark.parametrize("E", [1, 5, 128])
def test_segment_column_sums(E, N):
    KC = _kc()
    counts_l, offsets_l = _colsum_table(E)
    R = offsets_l[-1] + 5
    counts, offsets = torch.tensor(counts_l, dtype=I32), torch.tensor(offsets_l, dtype=I32)
    live = CO.row_experts(counts, offsets, R) >= 0
    g = torch.Generator().manual_seed(E + N)
    x = torch.randn(R, N, generator=g).to(BF16)
    x[~live] = 1.0e4  # padding rows must influence nothing
    exact = CO.segment_colsum(x, counts, offsets)
    ref = torch.stack([x[o : o + c].sum(dim=0) for c, o in zip(counts_l, offsets_l)])  # torch's bf16 sum: the reference's bias gradient
    xv, xbuf = _padded(x.cuda())
    cd, od = counts.cuda(), offsets.cuda()
    empty = [e for e, c in enumerate(counts_l) if c == 0]
    bad = []
    for dtype in (BF16, F32):
        def fresh(fill):
            buf = torch.full((E, 1, N + 8), SENT, dtype=dtype, device="cuda")  # the arena's layout: other parameters between two experts' biases
            buf[:, :, :N] = fill
            return buf[:, :, :N], buf

        out, buf = fresh(3.0)
        KC.segment_colsum(xv, cd, od, out)
        assert bool((buf[:, :, N:] == SENT).all()) and _guards_untouched(xbuf, R, N)
        for e in empty:
            assert bool((out[e] == 0).all()), "an expert without a row gets exactly zero"
        judge(f"sums ({dtype})", out.view(E, N), ref if dtype == BF16 else ref.float(), exact, bad)
        if dtype == F32:  # one row: the row itself; fp32 sums of bf16 values against fp64: 3 000 additions of 2^-24 relative each
            assert E == 1 or torch.equal(out[1, 0], xv[offsets_l[1]].float())
            assert CO.rel_l2(out.view(E, N).cpu(), exact) <= 3000 * 2.0 ** -24
        out2, _ = fresh(3.0)
        KC.segment_colsum(xv, cd, od, out2)
        assert torch.equal(out, out2), "two calls differ"
        # accumulating: onto a previous gradient; an expert without a row keeps its bits, a -0.0 included
        prev = torch.randn(E, 1, N, generator=g).to(dtype)
        prev[:, 0, 0] = -0.0
        acc, buf = fresh(prev.cuda())
        KC.segment_colsum(xv, cd, od, acc, accumulate=True)
        assert bool((buf[:, :, N:] == SENT).all())
        for e in empty:
            assert torch.equal(acc[e].view(torch.int16 if dtype == BF16 else torch.int32), prev[e].cuda().view(torch.int16 if dtype == BF16 else torch.int32)), "untouched"
        want = (prev.view(E, N).float().cuda() + (out.view(E, N).float() if dtype == F32 else CO.segment_colsum(x, counts, offsets, dtype=F32).cuda()))
        judge(f"accumulated ({dtype})", acc.view(E, N), want.to(dtype), prev.view(E, N).double() + exact, bad)
    assert not bad, "\n".join(bad)


# ----------------------------------------------------------------------------------------------------------------- ExpertGeLU alone
@pytest.mark.parametrize("emb_dim", [16, 64])
def test_expert_on_its_own(emb_dim):
    from llm_quest_amd.moe.classic_moe import ExpertGeLU

    T = 33
    g = torch.Generator().manual_seed(emb_dim)
    r = lambda *shape, scale: (scale * torch.randn(*shape, generator=g)).to(BF16)
    ex = ExpertGeLU(dict(emb_dim=emb_dim), 0.625).to(BF16)  # hidden 40 / 160
    hidden = ex.hidden_dim
    assert hidden == int(2.5 * emb_dim)
    sd = {"layers.0.weight": r(hidden, emb_dim, scale=emb_dim ** -0.5), "layers.0.bias": r(hidden, scale=0.3),
          "layers.2.weight": r(emb_dim, hidden, scale=hidden ** -0.5), "layers.2.bias": r(emb_dim, scale=0.3)}
    x, dy = r(T, emb_dim, scale=1.0), r(T, emb_dim, scale=1.0)
    ex.load_state_dict(sd)
    ex = ex.cuda()
    xg = x.view(1, T, emb_dim).cuda().requires_grad_(True)
    y = ex(xg)
    y.backward(dy.view(1, T, emb_dim).cuda())
    names = ("layers.0.weight", "layers.0.bias", "layers.2.weight", "layers.2.bias")
    ops = [sd[n] for n in names]
    ref, exact = CO.expert_grads(x, *ops, dy), CO.expert_grads(x, *ops, dy, dtype=F64)
    mine = (y.view(T, emb_dim), xg.grad.view(T, emb_dim)) + tuple(dict(ex.named_parameters())[n].grad for n in names)
    bad = []
    for name, m_, r_, e_ in zip(("out", "dx") + tuple("d " + n for n in names), mine, ref, exact):
        judge(name, m_, r_, e_, bad)
    with torch.no_grad():
        y2 = ex(xg)
    assert torch.equal(y2, y) and y2.grad_fn is None
    with pytest.raises(RuntimeError):
        y2.sum().backward()
    with pytest.raises(TypeError, match="bf16"):
        ex(xg.detach().float())
    assert not bad, "\n".join(bad)


# ----------------------------------------------------------------------------------------------------------------- the layer on the fixture
@pytest.fixture(scope="module")
def fixture():
    return CO.load_fixture("classic_moe_tiny")


def _layer(name, t, forced=True, cls="MoE"):
    from llm_quest_amd.moe import classic_moe as M

    spec, pre = CO.FIXTURE_LAYERS[name], name + "."
    m = getattr(M, cls)(dict(spec["cfg"]), **spec["kwargs"]).to(BF16)
    m.load_state_dict({n[len(pre + "sd."):]: v for n, v in t.items() if n.startswith(pre + "sd.")})
    m = m.cuda().train()
    if forced:
        m._forced_topk = t[pre + "topk_idxs"].cuda()
    return m


def _step(m, x, dout, g):
    """One training forward + the fixture's total (out * dout).sum() + g * moe_loss + backward -> (out, moe_loss, dx, {name: gradient})."""
    xg = x.cuda().requires_grad_(True)
    out = m(xg)
    loss = m.moe_loss
    assert loss.dim() == 0 and loss.dtype == BF16 and loss.requires_grad
    ((out * dout.cuda()).sum() + g * loss).backward()
    return out.detach(), loss.detach(), xg.grad, {n: p.grad for n, p in m.named_parameters()}


@pytest.mark.parametrize("name", list(CO.FIXTURE_LAYERS))
def test_layer_on_the_fixture(name, fixture):
    t, spec, pre = fixture, CO.FIXTURE_LAYERS[name], name + "."
    E = spec["E"]
    x, dout, g = t[pre + "in.x"], t[pre + "in.dout"], float(t[pre + "in.g"])
    m = _layer(name, t)
    out, loss, dx, grads = _step(m, x, dout, g)
    assert torch.equal(m._routed[0].cpu(), t[pre + "topk_idxs"]) and torch.equal(m._routed[1].cpu().long(), CO.counts_of(t[pre + "topk_idxs"].long(), E))
    bad = []
    judge("out", out, t[pre + "out"], t[pre + "twin.out"], bad)
    judge("moe_loss", loss, t[pre + "moe_loss"], t[pre + "twin.moe_loss"], bad)
    judge("dx", dx, t[pre + "grad.x"], t[pre + "twin.grad.x"], bad)
    lo, hi = m._arena.grad.data_ptr(), m._arena.grad.data_ptr() + m._arena.grad.numel() * 2
    for n, gr in grads.items():
        assert gr is not None and lo <= gr.data_ptr() < hi, n
        judge("d " + n, gr, t[pre + "grad." + n], t[pre + "twin.grad." + n], bad)
    # the no-grad forward gives the training forward's bits and sets moe_loss too; no backward through it; MoE_old computes the same function
    with torch.no_grad():
        out2 = m(x.cuda())
    assert torch.equal(out2, out) and out2.grad_fn is None and torch.equal(m.moe_loss, loss) and not m.moe_loss.requires_grad
    with pytest.raises(RuntimeError):
        out2.sum().backward()
    m.eval()
    with torch.no_grad():
        assert torch.equal(m(x.cuda()), out) and torch.equal(m.moe_loss, loss)
    old = _layer(name, t, cls="MoE_old")
    out3, loss3, dx3, grads3 = _step(old, x, dout, g)
    assert torch.equal(out3, out) and torch.equal(loss3, loss) and torch.equal(dx3, dx) and all(torch.equal(grads3[n], grads[n]) for n in grads)
    # the loss alone is differentiable: only the gate receives a gradient from it
    only = _layer(name, t)
    xg = x.cuda().requires_grad_(True)
    only(xg)
    only.moe_loss.backward()
    assert float(only.gate.weight.grad.float().abs().max()) > 0 and float(only.gate.bias.grad.float().abs().max()) > 0 and float(xg.grad.float().abs().max()) > 0
    assert all(bool((p.grad == 0).all()) for n, p in only.named_parameters() if n.startswith("experts."))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", list(CO.FIXTURE_LAYERS))
def test_segmented_and_per_expert_paths_give_the_same_bits(name, fixture, switch):
    t, pre = fixture, name + "."
    res = {}
    for on in (True, False):
        switch(on)
        res[on] = _step(_layer(name, t), t[pre + "in.x"], t[pre + "in.dout"], float(t[pre + "in.g"]))
    assert torch.equal(res[True][0], res[False][0]), "out"
    assert torch.equal(res[True][1], res[False][1]), "moe_loss"
    assert torch.equal(res[True][2], res[False][2]), "dx"
    for n, g in res[True][3].items():
        assert g is not None and res[False][3][n] is not None and torch.equal(g, res[False][3][n]), n


@pytest.mark.parametrize("segmented", [True, False], ids=["segmented", "per-expert"])
def test_a_routing_that_leaves_experts_empty(segmented, switch):
    from llm_quest_amd.moe.classic_moe import MoE

    switch(segmented)
    used, T = (2, 5, 9), 70
    torch.manual_seed(40)
    m = MoE(dict(emb_dim=64), num_experts=12, top_k=3, scaling_factor=0.125).to(BF16).cuda().train()
    m._forced_topk = torch.stack([torch.tensor(used).roll(i % 3) for i in range(T)]).to(I32).cuda()
    gen = torch.Generator().manual_seed(41)
    x, dout = torch.randn(2, 35, 64, generator=gen).to(BF16), torch.randn(2, 35, 64, generator=gen).to(BF16)
    out, loss, dx, grads = _step(m, x, dout, 1.0)
    assert m._routed[1].tolist() == [T if e in used else 0 for e in range(12)]
    once = {n: g.clone() for n, g in grads.items()}
    for n, g in once.items():
        assert g is not None and bool(torch.isfinite(g.float()).all()), n
        if n.startswith("experts."):
            if int(n.split(".")[1]) in used:
                assert float(g.float().abs().max()) > 0, n
            else:
                assert bool((g == 0).all()), f"{n}: an expert without a token must have an exactly zero gradient"
    out2, loss2, dx2, twice = _step(m, x, dout, 1.0)  # no zero_grad in between: the second backward accumulates
    assert torch.equal(out2, out) and torch.equal(loss2, loss) and torch.equal(dx2, dx)
    for n, g in twice.items():
        if float(once[n].float().abs().max()) == 0.0:
            assert bool((g == 0).all()), n
        else:
            # bf16(s + bf16(s)) against 2 bf16(s), s the fp32 sum: |s - bf16(s)| <= 2^-8 |s| (bf16's unit roundoff) and one more rounding of about 2 s,
            # so at most 1.5 * 2^-8 relative per element, hence in the L2 norm
            assert CO.rel_l2(g.cpu(), once[n].double().cpu() * 2) <= 1.5 * 2.0 ** -8, n
    for p in m.experts[0].parameters():  # some but not all of the experts' parameters trainable: refused
        p.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="all be trainable or all frozen"):
        _step(m, x, dout, 1.0)


def test_twenty_optimizer_steps_lower_the_loss(fixture):
    from llm_quest_amd import ops
    from llm_quest_amd.optim import ArenaAdamW

    t = fixture
    m = _layer("B", t, forced=False)
    x, dout = t["B.in.x"].cuda(), t["B.in.dout"].cuda()
    ops.arena_for(m)
    opt = ArenaAdamW(m.parameters(), lr=1e-3, weight_decay=0.0).attach(m)
    totals = []
    for step in range(21):
        out = m(x)
        total = (out * dout).sum() + m.moe_loss
        totals.append(total.detach().float())
        if step == 20:
            break
        opt.zero_grad(set_to_none=True)
        total.backward()
        opt.step()
    totals = torch.stack(totals).cpu()
    print("  totals", [round(float(v), 4) for v in totals])
    assert bool(torch.isfinite(totals).all()) and float(totals[-1]) < float(totals[0])


# ----------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_come_back_as_codes_with_messages():
    from llm_quest_amd import _lib as L

    buf = torch.full((1 << 16,), 1.0, dtype=F32, device="cuda")  # every operand of every call; 1.0 is a value no kernel here would leave everywhere
    refusal_checks(L.load(), buf.data_ptr())
    torch.cuda.synchronize()
    assert bool((buf == 1.0).all()), "a refused call wrote to its operands"
    KC = _kc()
    x = torch.zeros(4, 8, dtype=BF16, device="cuda")
    i32 = lambda *v: torch.tensor(v, dtype=I32, device="cuda")
    with pytest.raises(ValueError, match="top_k"):
        KC.route_fwd(x, 9)
    with pytest.raises(ValueError, match="num_experts"):
        KC.route_fwd(torch.zeros(4, 129, dtype=BF16, device="cuda"), 2)
    with pytest.raises(ValueError, match="logits must be bf16"):
        KC.route_fwd(x.float(), 2)
    with pytest.raises(ValueError, match="forced idx"):
        KC.route_fwd(x, 2, forced_idx=torch.zeros(4, 3, dtype=I32, device="cuda"))
    with pytest.raises(ValueError, match="needs the counts and lse"):
        KC.route_bwd(torch.zeros(4, 2, device="cuda"), torch.zeros(4, 2, dtype=BF16, device="cuda"), torch.ones(4, device="cuda"), torch.zeros(4, 2, dtype=I32, device="cuda"), x,
                     g=torch.ones(1, device="cuda"))
    with pytest.raises(ValueError, match="multiple of 8"):
        KC.bias_act_fwd(torch.zeros(4, 12, dtype=BF16, device="cuda"), torch.zeros(1, 1, 12, dtype=BF16, device="cuda"), i32(4), i32(0, 32), True)
    with pytest.raises(ValueError, match=r"stack \[2, 1, 8\]"):
        KC.bias_act_fwd(x, torch.zeros(2, 1, 16, dtype=BF16, device="cuda"), i32(4, 0), i32(0, 32, 32), True)
    with pytest.raises(ValueError, match="counts must be contiguous int32"):
        KC.bias_act_fwd(x, torch.zeros(2, 1, 8, dtype=BF16, device="cuda"), i32(4), i32(0, 32, 32), True)
    with pytest.raises(ValueError, match=r"stack \[1, 1, 8\]"):
        KC.segment_colsum(x, i32(4), i32(0, 32), torch.zeros(1, 1, 16, device="cuda"))
