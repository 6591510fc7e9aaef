"""The mixture-of-experts layers on the segmented GEMMs (``ops_moe.SEGMENTED``, the default): no device-to-host read in forward + backward, a launch
count that does not depend on the number of experts, and every output and gradient of ``Qwen3MoE`` and ``DeepSeekMoE`` against the restatements on
BOTH paths (the per-expert path stays covered now that the default moved).

Tolerance: the project's 1.5x rule (``judge`` of test_moe_gpu.py).  Counts and sentinels are compared exactly.
"""

import collections
import json
import os

import pytest
import torch
import torch.nn.functional as F

import moe_oracle as MO
import test_deepseek_moe_gpu as TD
import test_moe_gpu as TM
from test_moe_gpu import judge

pytestmark = pytest.mark.gpu
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


@pytest.fixture
def switch(monkeypatch):
    """Sets ``ops_moe.SEGMENTED`` for one test (both layers read it there)."""
    from llm_quest_amd import ops_moe

    def set_(on):
        monkeypatch.setattr(ops_moe, "SEGMENTED", bool(on))

    return set_


# ----------------------------------------------------------------------------------------------------------------- host synchronisation
def _qwen_layer():
    c = TM.layer_case(*TM.LAYERS[0])
    moe = TM.build_layer(c)
    x, dy = c["x"].cuda().unsqueeze(0), c["dy"].cuda().unsqueeze(0)
    one = torch.ones((), dtype=BF16, device="cuda")

    def step():
        xg = x.detach().requires_grad_(True)
        out = moe(xg)
        torch.autograd.backward([out, moe.moe_loss], [dy, one])
        return xg.grad

    return step


def _qwen_block():
    from llm_quest_amd import ops
    from llm_quest_amd.qwen.qwen3.qwen3_model import Qwen3MoEModel

    cfg = dict(MO.TINY_MOE)
    torch.manual_seed(5)
    m = Qwen3MoEModel(cfg).cuda().train()
    blk = m.trf_blocks[0]
    B, S, d = 2, 48, cfg["emb_dim"]
    x = torch.randn(B, S, d, generator=torch.Generator().manual_seed(6)).to(BF16).cuda()
    dy = torch.randn(B, S, d, generator=torch.Generator().manual_seed(7)).to(BF16).cuda()
    rt = ops.make_runtime(B, S, x.device, m.cos, m.sin, None, None)
    one = torch.ones((), dtype=BF16, device="cuda")

    def step():
        xg = x.detach().requires_grad_(True)
        out = blk(xg, m.mask, m.cos, m.sin, _runtime=rt)
        torch.autograd.backward([out, blk.moe.moe_loss], [dy, one])
        return xg.grad

    return step


def _deepseek_layer():
    from llm_quest_amd.moe.deepseek_moe import DeepSeekMoE

    cfg, T = TD._layer_cfg("7 routed + 1 shared, k 3, T 70")
    torch.manual_seed(8)
    moe = DeepSeekMoE(cfg).to(BF16).cuda().train()
    x = torch.randn(1, T, 64, generator=torch.Generator().manual_seed(9)).to(BF16).cuda()
    dy = torch.randn(1, T, 64, generator=torch.Generator().manual_seed(10)).to(BF16).cuda()

    def step():
        xg = x.detach().requires_grad_(True)
        moe(xg).backward(dy)
        return xg.grad

    return step


def _deepseek_block():
    import deepseek_moe_oracle as DMO
    from llm_quest_amd import ops_mla
    from llm_quest_amd.llama3_to_deepseekv3.deepseek_model import DeepSeekV3Model
    from llm_quest_amd.moe.deepseek_moe import DeepSeekMoE

    cfg = dict(DMO.TINY_DEEPSEEK_MOE)
    torch.manual_seed(11)
    m = DeepSeekV3Model(cfg).to(BF16).cuda().train()
    blk = [b for b in m.main_model.trf_blocks if isinstance(b.ffn, DeepSeekMoE)][0]
    B, S, d = 2, 24, cfg["emb_dim"]
    x = torch.randn(B, S, d, generator=torch.Generator().manual_seed(12)).to(BF16).cuda()
    dy = torch.randn(B, S, d, generator=torch.Generator().manual_seed(13)).to(BF16).cuda()
    rt = ops_mla.make_runtime(m, B, S, m.cos, m.sin)

    def step():
        xg = x.detach().requires_grad_(True)
        blk(xg, m.mask, m.cos, m.sin, _runtime=rt).backward(dy)
        return xg.grad

    return step


def test_forward_and_backward_never_synchronise_with_the_host(switch):
    """Under torch's sync debug mode "error" every device-to-host read raises.  The four subjects (both layers, both blocks) run one warm-up step outside
    the mode (library load, arena, workspaces), then a whole forward + backward inside it.  With the switch off the Qwen3MoE layer reads its counts: it
    must raise, which also shows that the mode sees this path's reads."""
    switch(True)
    steps = {"Qwen3MoE": _qwen_layer(), "MoETransformerBlock": _qwen_block(), "DeepSeekMoE": _deepseek_layer(), "DeepSeek MoE block": _deepseek_block()}
    want = {n: s().clone() for n, s in steps.items()}  # warm-up, and the values to meet again
    probe = torch.ones(1, device="cuda")
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        bites = False
        try:
            probe.item()
        except RuntimeError:
            bites = True
        if not bites:
            pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on .item() in this build: the host reads cannot be observed")
        got = {n: s() for n, s in steps.items()}
        switch(False)
        with pytest.raises(RuntimeError):
            steps["Qwen3MoE"]()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    for n in steps:
        if n.startswith("DeepSeek"):  # (its forward moves the router's biases: the second step may route differently)
            assert bool(torch.isfinite(got[n].float()).all()), n
        else:
            assert torch.equal(got[n], want[n]), n


# ----------------------------------------------------------------------------------------------------------------- launch count
def _counted(step):
    """The entry-point name of every ``L.call`` that ``step()`` makes, in order.  ``L.call`` is put back whether ``step`` returns or raises."""
    from llm_quest_amd import _lib as L

    names, real = [], L.call

    def counting(name, *args):
        names.append(name)
        return real(name, *args)

    L.call = counting
    try:
        step()
    finally:
        L.call = real
    return names


def _qwen_launch_step(E):
    from llm_quest_amd.moe.qwen3_moe import Qwen3MoE

    torch.manual_seed(20 + E)
    moe = Qwen3MoE(dict(emb_dim=64, moe_hidden_dim=64, num_experts=E, top_k=2, aux_loss_coef=0.01, dtype=BF16)).cuda().train()
    x = torch.randn(1, 70, 64, generator=torch.Generator().manual_seed(21)).to(BF16).cuda().requires_grad_(True)

    def step():
        out = moe(x)
        torch.autograd.backward([out, moe.moe_loss], [torch.ones_like(out), torch.ones((), dtype=BF16, device="cuda")])
        assert all(p.grad is not None for p in moe.parameters())

    return step


def _count_calls(E):
    return _counted(_qwen_launch_step(E))


def test_launch_count_does_not_depend_on_the_number_of_experts(switch):
    switch(True)
    n8, n16 = _count_calls(8), _count_calls(16)
    print(f"  {len(n8)} calls at E = 8, {len(n16)} at E = 16: {sorted(set(n8))}")
    assert n8 == n16
    for names in (n8, n16):
        assert names.count("mi355_gemm_bf16") == 2  # the gate's logits and its dgrad: no per-expert product
        assert names.count("mi355_gemm_bf16_segmented") == 4 and names.count("mi355_gemm_bf16_segmented_tn") == 2
        assert names.count("mi355_gemm_bf16_grouped") == 1  # the gate's weight gradient
    switch(False)
    off8, off16 = _count_calls(8), _count_calls(16)
    assert len(off16) > len(off8) > len(n8) and "mi355_gemm_bf16_segmented" not in off8


# ----------------------------------------------------------------------------------------------------------------- the recorded launches
LAUNCH_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "moe_launches.json")  # written by tools/record_moe_launches.py
PATHS = {"segmented": True, "per-expert": False}


def _latent_launch_step(name):
    import latent_moe_oracle as LO
    import test_latent_moe_gpu as TL

    t = LO.load_fixture("latent_moe_tiny")
    m = TL._layer(name, t)
    return lambda: TL._step(m, t[name + ".in.x"])


def _classic_launch_step(name):
    import classic_moe_oracle as CO
    import test_classic_moe_gpu as TC

    t, pre = CO.load_fixture("classic_moe_tiny"), name + "."
    m = TC._layer(name, t)
    return lambda: TC._step(m, t[pre + "in.x"], t[pre + "in.dout"], float(t[pre + "in.g"]))


# one forward + backward (the loss included where the layer has one) of every mixture-of-experts layer on the fixtures' own tiny shapes: T = 70 tokens,
# widths 64 to 80; a padded (E = 12, 3, 7) and an unpadded (E = 16, 8, 8) gate, fp32 (LatentMoE A) and bf16 balancing biases
LAUNCH_CASES = {
    "LatentMoE A": lambda: _latent_launch_step("A"),
    "LatentMoE B": lambda: _latent_launch_step("B"),
    "classic MoE A": lambda: _classic_launch_step("A"),
    "classic MoE B": lambda: _classic_launch_step("B"),
    "DeepSeekMoE 7 routed + 1 shared, k 3, T 70": lambda: _deepseek_layer(),
    "Qwen3MoE E 8": lambda: _qwen_launch_step(8),
}


def launch_counts(case, segmented):
    """{entry point: number of calls} of the first forward + backward of a freshly built layer, with ``ops_moe.SEGMENTED`` set to ``segmented``."""
    from llm_quest_amd import ops_moe

    before = ops_moe.SEGMENTED
    ops_moe.SEGMENTED = bool(segmented)
    try:
        return dict(sorted(collections.Counter(_counted(LAUNCH_CASES[case]())).items()))
    finally:
        ops_moe.SEGMENTED = before


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("case", list(LAUNCH_CASES))
def test_every_layer_issues_the_recorded_launches(case, path):
    """The host layer may be reorganised, the launches may not change: per entry point, as many calls as tests/golden/moe_launches.json records."""
    with open(LAUNCH_GOLDEN) as f:
        want = json.load(f)[case][path]
    got = launch_counts(case, PATHS[path])
    print(f"  {case}, {path}: {sum(got.values())} calls")
    assert got == want, {n: (got.get(n, 0), want.get(n, 0)) for n in sorted(set(got) | set(want)) if got.get(n, 0) != want.get(n, 0)}


# ----------------------------------------------------------------------------------------------------------------- layers, both paths
def _judge_qwen(c, mine, E, empty):
    bad = []
    for name in ("out", "loss", "p", "dx", "gate.weight") + tuple(f"experts.{e}.{l}.weight" for e in range(E) for l in ("lin1", "lin_gate", "lin2")):
        assert mine[name] is not None, name
        judge(name, mine[name], c[None][name], c[torch.float64][name], bad)
    for e in empty:
        for l in ("lin1", "lin_gate", "lin2"):  # an expert without a token: a defined, exactly zero gradient
            gr = mine[f"experts.{e}.{l}.weight"]
            assert gr is not None and float(gr.float().abs().max()) == 0.0, (e, l)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("segmented", [True, False], ids=["segmented", "per-expert"])
@pytest.mark.parametrize("T,d,F_", TM.LAYERS)
def test_qwen3_layer_against_the_restatement_on_both_paths(T, d, F_, segmented, switch):
    switch(segmented)
    c = TM.layer_case(T, d, F_)
    _judge_qwen(c, TM.run_layer(c, TM.build_layer(c)), 8, [TM.EMPTY])


@pytest.mark.parametrize("segmented", [True, False], ids=["segmented", "per-expert"])
@pytest.mark.parametrize("name", list(TD.LAYER_CASES))
def test_deepseek_layer_against_the_restatement_on_both_paths(name, segmented, switch):
    c = TD._layer_run(name)  # the restatement's two flows on the selection the kernels made (the router does not depend on the switch)
    switch(segmented)
    moe, y, dx = c["run"]()
    assert torch.equal(moe._routed[0].cpu().long(), c["idx"]) and torch.equal(moe._routed[1].cpu().long(), c["counts"])
    bad = []
    TD.judge("out", y, c["ref"][0], c["exact"][0], bad)
    TD.judge("dx", dx, c["ref"][1], c["exact"][1], bad)
    grads = TD._grads_of(moe)
    assert set(grads) == set(c["ref"][2])
    for n, g in grads.items():
        assert g is not None, n
        TD.judge("d " + n, g, c["ref"][2][n], c["exact"][2][n], bad)
        if n.startswith("routed_experts.") and int(c["counts"][int(n.split(".")[1])]) == 0:
            assert bool((g == 0).all()), f"{n}: an expert without a token must have an exactly zero gradient"
    assert not bad, "\n".join(bad)


def test_second_backward_accumulates_and_mixed_gradient_states_resolve(switch):
    """Two backward passes without zero_grad add up; with some experts' gradients dropped in between (``.grad = None``) the dropped ones restart
    from zero and the others keep accumulating -- ``arena.grad_target`` over the experts' range decides, as on the per-expert path."""
    c = TM.layer_case(*TM.LAYERS[0])
    res = {}
    for on in (True, False):
        switch(on)
        moe = TM.build_layer(c)
        TM.run_layer(c, moe)
        moe.experts[2].lin2.weight.grad = None
        moe.experts[3].lin1.weight.grad = None
        r = TM.run_layer(c, moe)
        res[on] = {n: g.clone() for n, g in r.items() if n.startswith("experts.")}
    once = {n: g for n, g in TM.run_layer(c, TM.build_layer(c)).items() if n.startswith("experts.")}
    for n, g in res[True].items():
        if float(once[n].float().abs().max()) == 0.0:  # the expert without a token stays exactly zero
            assert float(g.float().abs().max()) == 0.0 and float(res[False][n].float().abs().max()) == 0.0, n
        elif n in ("experts.2.lin2.weight", "experts.3.lin1.weight"):  # restarted: 0 + the product, rounded once -- the single run's bits
            assert torch.equal(g, once[n]), n
        else:
            # bf16(s + bf16(s)) against 2 bf16(s), s the fp32 sum: |s - bf16(s)| <= 2^-8 |s| (bf16's unit roundoff) and one more rounding of about 2 s,
            # so at most 1.5 * 2^-8 relative per element, hence in the L2 norm
            assert MO.rel_l2(g, once[n].double() * 2) <= 1.5 * 2.0 ** -8, n
        assert MO.rel_l2(g, res[False][n]) <= 2.0 ** -7 or float(g.float().abs().max()) == 0.0, n  # the two paths round the same sums: a bf16 ulp (2^-7 relative) apart at most


# ----------------------------------------------------------------------------------------------------------------- a wider layer
WIDE = dict(E=16, k=4, T=70, d=136, F=96, empty=(2, 7, 13), candidates=16)
_WIDE = {}


def wide_case():
    """``layer_case`` of test_moe_gpu.py (same gate scaling, same token rejection rule, same assertion that enough rows survive) at E = 16, k = 4, T = 70,
    d = 136 (K tails of 8 behind two 64-wide K-tiles), F = 96 (the fused SwiGLU path; 2F = 192 columns: one and a half column tiles), with three experts
    forced empty by the -10 gate column."""
    if _WIDE:
        return _WIDE
    E, k, T, d, F_, empty = (WIDE[n] for n in ("E", "k", "T", "d", "F", "empty"))
    cfg = dict(emb_dim=d, moe_hidden_dim=F_, num_experts=E, top_k=k, aux_loss_coef=0.01, dtype=BF16)
    g = torch.Generator().manual_seed(300 + T + d + F_ + E)
    u = lambda rows, cols: ((torch.rand(rows, cols, generator=g) * 2 - 1) / cols ** 0.5).to(BF16)
    sd = {"gate.weight": (4 * u(E, d).float()).to(BF16)}
    sd["gate.weight"][:, 0] = 0.0
    for e in empty:
        sd["gate.weight"][e, 0] = -10.0
    for e in range(E):
        sd[f"experts.{e}.lin1.weight"], sd[f"experts.{e}.lin_gate.weight"], sd[f"experts.{e}.lin2.weight"] = u(F_, d), u(F_, d), u(d, F_)
    n_cand = WIDE["candidates"] * T
    cand = torch.randn(n_cand, d, generator=g).to(BF16)
    cand[:, 0] = 4.0
    lg = {dt: F.linear(MO._c(cand, dt), MO._c(sd["gate.weight"], dt)) for dt in (None, torch.float64)}
    keep = torch.ones(n_cand, dtype=torch.bool)
    sel = {}
    for dt in (None, torch.float64):
        pv, pi = MO.topk_lowest_index_first(F.softmax(lg[dt], dim=-1), k + 1)
        keep &= (pv[:, k - 1].double() / pv[:, k].double() >= 1.25) & (lg[dt].gather(1, pi).abs().max(dim=1)[0] < 8)
        sel[dt] = pi[:, :k].sort(dim=1)[0]
    keep &= (sel[None] == sel[torch.float64]).all(dim=1)
    assert int(keep.sum()) >= T, "the rejection left too few token rows"
    x = cand[keep][:T].contiguous()
    dy = torch.randn(T, d, generator=g).to(BF16)
    c = {"cfg": cfg, "sd": sd, "x": x, "dy": dy, "g": 3.0}
    for dt in (None, torch.float64):
        leaves = {n: MO._c(v, dt).detach().requires_grad_(True) for n, v in sd.items()}
        xg = MO._c(x, dt).detach().requires_grad_(True)
        out, p, loss, idx = MO.moe_layer(leaves, "", xg, cfg)
        names = list(leaves)
        grads = torch.autograd.grad((out * MO._c(dy, out.dtype)).sum() + c["g"] * loss, [xg] + [leaves[n] for n in names], allow_unused=True)
        r = dict(out=out.detach(), loss=loss.detach(), p=p.detach(), idx=idx, dx=grads[0])
        r.update({n: (torch.zeros_like(leaves[n]) if gr is None else gr) for n, gr in zip(names, grads[1:])})
        c[dt] = r
    assert torch.equal(c[None]["idx"].sort(dim=1)[0], c[torch.float64]["idx"].sort(dim=1)[0])
    assert not any(bool((c[None]["idx"] == e).any()) for e in empty)
    _WIDE.update(c)
    return _WIDE


@pytest.mark.parametrize("segmented", [True, False], ids=["segmented", "per-expert"])
def test_wide_layer_with_three_empty_experts(segmented, switch):
    switch(segmented)
    c = wide_case()
    _judge_qwen(c, TM.run_layer(c, TM.build_layer(c)), WIDE["E"], WIDE["empty"])
