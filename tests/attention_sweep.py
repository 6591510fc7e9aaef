"""The fp64 sweep of the attention forward and backward (csrc/attention.hip): operands, the two reference flows, an fp32 emulation of the
kernels' rounding points, and the per-block judgement shared by test_attention_sweep_gpu.py and test_attention_sweep_cpu.py.
TEST INFRASTRUCTURE ONLY.

Reference flows (``oracle.ops.gqa_attention_core`` on [B, H, S, D] tensors, gradients by autograd):
  * on the bf16 operands as given it is the reference's arithmetic; its distance to the fp64 result is the FLOOR of a block;
  * on the operands upcast to fp64 it is the EXACT value every implementation is measured against.

Judgement (``judge``): o, dq, dk, dv are cut into blocks of 32 consecutive tokens per (sample, head) -- the smallest unit one wave owns; a ragged
tail shorter than 32 joins the block before it.  A block passes when rel_l2(kernel, exact) <= max(1.5 * floor of that block, cap), and the whole
tensor must satisfy the same formula.  The caps are the numbers the suite applies to whole tensors (test_kernels_gpu.py): 4e-3 for o, 8e-3 for the
gradients.  (The plain 1.5 x floor + 2e-3 rule of the side kernels is not usable at tiny S, where the floor is near zero.)  Token rows whose exact
value is identically zero have no relative distance: dk / dv of padded keys and dq of fully-masked rows must be exactly 0.  A one-key softmax has
dS = P (dP - delta) with dP = dO . v and delta = dO . o, so dq of a row that sees one key is bounded by one rounding of o entering delta,
|dq_d| <= 2^-7 * scale * sum_e |dO_e v_e| * |k_d|.  dk of a key that only such rows see has the mirror image as its bound: at S = 1, and for
every key of a window of one in tests/side_attention_sweep.py (``one_key_bounds``).  No block is left out: ``judge`` counts the blocks it judged
and the blocks there are, and a zero block whose rows have no rule of their own is a failure.
"""

import math

import torch

BF16 = torch.bfloat16
CAP = {"o": 4e-3, "dq": 8e-3, "dk": 8e-3, "dv": 8e-3}
LSE_TOL = 6e-3  # |lse - lse_ref| on rows with a visible key (test_attention_forward_second_generation_matches_fp64)
O_CAP_ONE_KEY = 2.0 ** -7  # o of the one-row, one-key block at S = 1 (derived in ``judge``)
LSE_FILL = -2.0e38 * 0.6931471805599453  # the kernel's finite fill in natural-log units
BLOCK = 32

SWEEP_S = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 193, 255, 256, 257, 385)
SWEEP_HEADS = ((2, 1, 128), (8, 1, 128), (2, 2, 128), (3, 3, 64), (4, 1, 64))  # Hq, Hkv, D
MASKS = ("none", "right", "holes", "left")


def sweep_cases():
    """(B, S, Hq, Hkv, D, causal, mask) of the edge grid.  The mask kind rotates with the case index: for a fixed S the five head shapes, and for a
    fixed head shape the sixteen lengths, walk through all four kinds."""
    out = []
    for si, S in enumerate(SWEEP_S):
        for hi, (Hq, Hkv, D) in enumerate(SWEEP_HEADS):
            for ci, causal in enumerate((True, False)):
                out.append((2 if S <= 200 else 1, S, Hq, Hkv, D, causal, MASKS[(si + hi + ci) % 4]))
    return out


def case_id(c):
    B, S, Hq, Hkv, D, causal, mask = c
    return f"B{B}-S{S}-H{Hq}x{Hkv}-D{D}-{'causal' if causal else 'full'}-{mask}"


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def to_tokens(x):
    """[B, H, S, D] -> [B*S, H*D]"""
    B, H, S, D = x.shape
    return x.transpose(1, 2).reshape(B * S, H * D).contiguous()


def from_tokens(x, B, S, H, D):
    return x.reshape(B, S, H, D).transpose(1, 2)


def operands(B, S, Hq, Hkv, D, seed):
    """q, k, v, do as bf16 [B, H, S, D], N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda h: torch.randn(B, h, S, D, generator=g).to(BF16)
    return rn(Hq), rn(Hkv), rn(Hkv), rn(Hq)


def key_mask(kind, B, S):
    """uint8 [B, S] (1 = real token) or None: ``right`` pads the last third of sample 0, ``left`` its first third, ``holes`` every fifth key."""
    if kind == "none":
        return None
    km = torch.ones(B, S, dtype=torch.uint8)
    if kind == "right":
        km[0, S - S // 3 :] = 0
    elif kind == "left":
        km[0, : S // 3] = 0
    elif kind == "holes":
        km[:, 2::5] = 0
    else:
        raise ValueError(kind)
    return km


def blocked_pairs(B, S, km, causal):
    """bool [B, 1, S, S]: True where query i may not see key j."""
    blocked = torch.zeros(B, 1, S, S, dtype=torch.bool)
    if causal:
        blocked = blocked | torch.ones(S, S, dtype=torch.bool).triu_(1)
    if km is not None:
        blocked = blocked | ~km.bool()[:, None, None, :]
    return blocked


def fully_masked_rows(B, S, km, causal):
    """bool [B, S]: queries whose visible keys are all padding."""
    return blocked_pairs(B, S, km, causal).all(dim=-1)[:, 0]


def reference(q, k, v, do, km, causal, dtype=None):
    """-> dict(o, dq, dk, dv) of ``gqa_attention_core`` and its autograd, on the tensors as given (``dtype=None``: the reference's arithmetic) or
    upcast to ``dtype`` first (fp64: the exact value)."""
    from oracle import ops

    c = lambda t: t if dtype is None else t.to(dtype)
    qr, kr, vr = (c(t).detach().requires_grad_(True) for t in (q, k, v))
    o = ops.gqa_attention_core(qr, kr, vr, q.shape[1] // k.shape[1], key_mask=km, causal=causal)
    dq, dk, dv = torch.autograd.grad(o, (qr, kr, vr), c(do))
    return {"o": o.detach(), "dq": dq, "dk": dk, "dv": dv}


def lse_reference(q, k, km, causal):
    """fp64 log-sum-exp of the masked, scaled scores with the kernel's fill -> (lse [B, Hq, S], live [B, Hq, S]: rows with a visible key)."""
    B, Hq, S, D = q.shape
    kx = k.double()[:, torch.arange(Hq) // (Hq // k.shape[1])]
    blocked = blocked_pairs(B, S, km, causal)
    sc = (q.double() @ kx.mT) * D ** -0.5
    return torch.logsumexp(sc.masked_fill(blocked, LSE_FILL), dim=-1), ~blocked.expand(B, Hq, S, S).all(dim=-1)


def uniform_dv_term(do, km, causal, Hkv):
    """What the backward's contract leaves out of dV: (1/S) * sum of dO over the fully-masked rows of the group's heads, for every key of the sample.
    do [B, Hq, S, D] -> fp64 [B, Hkv, S, D]."""
    B, Hq, S, D = do.shape
    dead = fully_masked_rows(B, S, km, causal)  # [B, S]
    t = (do.double() * dead[:, None, :, None]).sum(dim=2) / S  # [B, Hq, D]
    return t.view(B, Hkv, Hq // Hkv, D).sum(dim=2)[:, :, None, :].expand(B, Hkv, S, D)


# ----------------------------------------------------------------------------------------------------------------- the emulation
def emulate(q, k, v, do, km, causal, fold):
    """fp32 emulation of the kernels' rounding points, flash form: bf16 operands, fp32 scores and statistics, P and dS rounded to bf16 before they
    enter a product, bf16 outputs, masked pairs at probability 0 in the backward (a fully-masked row contributes nothing).  ``fold``: the scale is
    folded into a bf16 operand (the query rows in the forward, the key rows in the dK/dV pass), as the lean forward and the spill-form dK/dV pass do.
    -> dict(o, lse, dq, dk, dv)."""
    B, Hq, S, D = q.shape
    Hkv = k.shape[1]
    src = torch.arange(Hq) // (Hq // Hkv)
    scale = D ** -0.5
    r = lambda t: t.to(BF16).float()
    qf, kf, vf, dof = q.float(), k.float()[:, src], v.float()[:, src], do.float()
    blocked = blocked_pairs(B, S, km, causal)
    s = (r(qf * scale) @ kf.mT) if fold else (qf @ kf.mT) * scale
    sm = s.masked_fill(blocked, LSE_FILL)
    m = sm.max(dim=-1, keepdim=True).values
    p = torch.exp(sm - m)
    l = p.sum(dim=-1, keepdim=True)
    o = ((r(p) @ vf) / l).to(BF16)
    lse = (m + torch.log(l)).squeeze(-1)
    delta = (dof * o.float()).sum(dim=-1, keepdim=True)
    sb = (qf @ r(kf * scale).mT) if fold else s
    pb = torch.exp(sb - lse.unsqueeze(-1)).masked_fill(blocked, 0.0)
    ds = r(pb * (dof @ vf.mT - delta))
    group = lambda t: t.view(B, Hkv, Hq // Hkv, S, D).sum(dim=2)
    return {"o": o, "lse": lse, "dq": ((ds @ kf) * scale).to(BF16), "dk": group((ds.mT @ qf) * scale).to(BF16), "dv": group(r(pb).mT @ dof).to(BF16)}


# ----------------------------------------------------------------------------------------------------------------- the judgement
def block_edges(S):
    """Blocks of 32 tokens; a ragged tail shorter than 32 joins the block before it."""
    n = max(1, S // BLOCK)
    return [(i * BLOCK, S if i == n - 1 else (i + 1) * BLOCK) for i in range(n)]


def n_blocks(B, H, S):
    return B * H * len(block_edges(S))


def _block_norms(x, S):
    """x fp64 [B, H, S, D] -> squared norms [B, H, number of blocks]"""
    rows = x.pow(2).sum(dim=-1)
    return torch.stack([rows[..., a:b].sum(dim=-1) for a, b in block_edges(S)], dim=-1)


def judge_tensor(name, got, exact, floor, structural=None, one_key=None, cap=None):
    """One of o / dq / dk / dv, all [B, H, S, D]: ``got`` the implementation, ``exact`` fp64, ``floor`` the reference's bf16 result.
    ``structural``: bool [B, H, S], the token rows that are zero by the mask alone (padded keys for dk / dv, fully-masked queries for dq): where the
    exact row is zero too, the implementation's must be exactly 0.  ``one_key``: (rows bool [B, H, S], limit fp64 [B, H, S, D]) -- the rows of a
    one-key softmax and the bound on their elements.  ``cap``: a number, or fp64 [B, H, number of blocks] where a class of blocks has a bound of its
    own (the whole tensor is then held to the blocks' caps combined with the weights of their norms).
    -> (worst block ratio, blocks judged, list of failure strings)."""
    cap = CAP[name] if cap is None else cap
    B, H, S, D = exact.shape
    got, exact, floor = got.double(), exact.double(), floor.double()
    fails = []
    if not bool(torch.isfinite(got).all()):
        bad = (~torch.isfinite(got)).nonzero()[0].tolist()
        return math.inf, 0, [f"{name}: not finite at (sample, head, token, feature) {bad}"]
    zero_row = (exact == 0).all(dim=-1)
    covered = torch.zeros_like(zero_row)  # zero rows that have a rule of their own
    if structural is not None:
        covered = structural & zero_row
        over = (got != 0).any(dim=-1) & covered
        if bool(over.any()):
            b, h, t = over.nonzero()[0].tolist()
            fails.append(f"{name}: sample {b}, head {h}, token {t} (block {min(t // BLOCK, len(block_edges(S)) - 1)}) must be exactly 0, max |x| = {float(got[b, h, t].abs().max()):.3e}")
    if one_key is not None:
        rows, lim = one_key
        rows = rows & zero_row & ~covered
        over = (got.abs() > lim) & rows[..., None]
        covered = covered | rows
        if bool(over.any()):
            b, h, t, d = over.nonzero()[0].tolist()
            fails.append(f"{name}: |{float(got[b, h, t, d]):.3e}| > {float(lim[b, h, t, d]):.3e} at the one-key row of sample {b}, head {h}, token {t}, feature {d}")
    err, ref, flo = _block_norms(got - exact, S).sqrt(), _block_norms(exact, S).sqrt(), _block_norms(floor - exact, S).sqrt()
    live = ref > 0  # a block that is identically zero is judged row by row above: every one of its rows must have had a rule
    for b, h, i in (~live).nonzero().tolist():
        t0, t1 = block_edges(S)[i]
        if not bool(covered[b, h, t0:t1].all()):
            fails.append(f"{name}: sample {b}, head {h}, block {i}: the exact block is zero and no rule covers it")
    caps = cap.to(ref.dtype).expand_as(ref) if torch.is_tensor(cap) else torch.full_like(ref, cap)
    bound = torch.maximum(1.5 * flo / ref.clamp_min(1e-300), caps)
    ratio = torch.where(live, err / ref.clamp_min(1e-300) / bound, torch.zeros_like(ref))
    for b, h, i in (ratio > 1).nonzero().tolist():
        fails.append(f"{name}: sample {b}, head {h}, block {i} (tokens {block_edges(S)[i]}): rel l2 {float(err[b, h, i] / ref[b, h, i]):.3e} > "
                     f"max(1.5 * {float(flo[b, h, i] / ref[b, h, i]):.3e}, {float(caps[b, h, i]):.0e})")
    worst = float(ratio.max())
    if bool(live.any()):  # the whole tensor under the same formula
        e, f, n = float((got - exact).norm()), float((floor - exact).norm()), float(exact.norm())
        if torch.is_tensor(cap):
            cap = float((caps * ref).norm()) / n
        whole = e / n / max(1.5 * f / n, cap)
        if whole > 1:
            fails.append(f"{name}: whole tensor rel l2 {e / n:.3e} > max(1.5 * {f / n:.3e}, {cap:.0e})")
        worst = max(worst, whole)
    return worst, int(ratio.numel()), fails


def one_key_bounds(q, k, v, do, km, causal, allowed=None):
    """The rows whose softmax runs over ONE key j (S = 1; the first query under the causal mask; the first query behind a padded head; every query
    of a window of one): P = 1, dS = dO . v_j - delta, delta = dO . o with o = v_j up to one bf16 rounding, so |dS| <= 2^-7 sum_e |dO_e v_je| (the
    bound test_attention_fullsize_invariants allows for that row) and |dq_d| <= scale |dS| |k_jd|.  A key j whose every query is such a row (S = 1;
    every key of a window of one) has the mirror image as its dk: the sum of scale |dS_i| |q_id| over those queries and its group's heads.
    ``allowed``: bool [B, S, S], True where query i sees key j, for masks that (km, causal) cannot state (it replaces them); v and do may be
    narrower or wider than q and k.
    -> {"dq": (rows [B, Hq, S], limit [B, Hq, S, D]), "dk": the same for [B, Hkv, S, D], present at S = 1 and wherever such a key exists}"""
    B, Hq, S, D = q.shape
    Hkv = k.shape[1]
    src = torch.arange(Hq) // (Hq // Hkv)
    seen = ~blocked_pairs(B, S, km, causal)[:, 0] if allowed is None else allowed  # [B, S, S]
    rows = seen.sum(dim=-1) == 1
    j = seen.int().argmax(dim=-1)[:, None, :, None]
    kj, vj = k.double()[:, src].gather(2, j.expand(B, Hq, S, D)), v.double()[:, src].gather(2, j.expand(B, Hq, S, v.shape[-1]))
    ds = 2.0 ** -7 * D ** -0.5 * (do.double() * vj).abs().sum(dim=-1, keepdim=True)
    out = {"dq": (rows[:, None, :].expand(B, Hq, S), ds * kj.abs())}
    lone = seen & rows[:, :, None]  # [B, query, key]: the query sees this key and no other
    keys = lone.any(dim=1) & ~(seen & ~rows[:, :, None]).any(dim=1)  # [B, S]: seen, and by one-key rows only
    if S == 1 or bool(keys.any()):
        lim = torch.einsum("bij,bhid->bhjd", lone.double(), ds * q.double().abs())
        out["dk"] = (keys[:, None, :].expand(B, Hkv, S), lim.view(B, Hkv, Hq // Hkv, S, D).sum(dim=2))
    return out


def judge(got, exact, floor, km, causal, ops, allowed=None):
    """``got`` / ``exact`` / ``floor``: dicts with o, dq, dk, dv [B, H, S, D] (a missing key of ``got`` is not judged); ``km`` / ``causal``: the mask
    of the case (the rows that must be exactly zero); ``ops`` = (q, k, v, do), for the bound of the one-key rows.  ``allowed``: bool [B, S, S], the
    pairs (query, key) that see each other, in place of (km, causal): a query that sees no key and a key that no query sees must be exactly zero.
    -> (worst ratio per tensor, blocks judged, blocks there are, failures)."""
    worst, judged, total, fails = {}, 0, 0, []
    one_key = one_key_bounds(*ops, km, causal, allowed)
    for name in ("o", "dq", "dk", "dv"):
        if name not in got:
            continue
        structural = None
        B, H, S, _ = exact[name].shape
        if allowed is not None:
            if name != "o":
                structural = (~allowed.any(dim=-1 if name == "dq" else 1))[:, None, :].expand(B, H, S)
        elif name == "dq":
            structural = fully_masked_rows(B, S, km, causal)[:, None, :].expand(B, H, S)
        elif name in ("dk", "dv") and km is not None:
            structural = (~km.bool())[:, None, :].expand(B, H, S)
        # o at S = 1, a block of ONE row over ONE key.  The exact row is v_j.  The lean forward measures a row's scores against a reference that moves
        # only when they outgrow it by 2^8 (attention.hip, "forward, lean softmax"), not against the row maximum, so P = 2^(s - ref) is some number in
        # [2^-8, 2^8], it is rounded to bf16 for the P V product while l sums the unrounded P, and o = bf16(v_j * bf16(P) / P): v_j moved by up to half a
        # bf16 ulp (2^-8 relative) and rounded again, i.e. elements one ulp off, up to 2^-7 relative -- with many keys these roundings average out, with
        # one they hit the whole row alike.  The 4e-3 cap cannot hold there: the bound of this block is 2^-7.  (Measured 5.43e-3 at P = 1.0041 ->
        # 1.0078, reproduced from these rounding points on the CPU to all printed digits)
        cap = O_CAP_ONE_KEY if name == "o" and S == 1 else None
        w, n, f = judge_tensor(name, got[name], exact[name], floor[name], structural, one_key.get(name), cap)
        worst[name] = w
        judged += n
        total += n_blocks(*exact[name].shape[:3])
        fails += f
    return worst, judged, total, fails


def judge_lse(lse, q, k, km, causal):
    """|lse - fp64 lse| < 6e-3 on every row with a visible key, except that a row with ONE visible key j may use what its rounding points admit where
    that is more: its lse IS its score, the lean forward folds log2(e) / sqrt(d) into the bf16 query row (one more rounding of every q_d, up to 2^-8
    relative), so |lse - ref| <= 2^-8 * scale * sum_d |q_d k_jd| (~3e-2 at D = 128) with nothing to average over; rows with more keys average
    these errors with weights P_j and keep the 6e-3.  (Measured 6.47e-3 on such a row, S = 31, D = 128, reproduced from bf16(q c) . k_j on the CPU to
    all printed digits)  -> (max |lse - ref| over the rows with several keys, the same over one-key rows, failures)"""
    B, Hq, S, D = q.shape
    ref, live = lse_reference(q, k, km, causal)
    if not bool(torch.isfinite(lse).all()):
        return math.inf, math.inf, ["lse: not finite"]
    seen = ~blocked_pairs(B, S, km, causal)[:, 0]
    one = (seen.sum(dim=-1) == 1)[:, None, :].expand(B, Hq, S)
    j = seen.int().argmax(dim=-1)[:, None, :, None].expand(B, Hq, S, D)
    kj = k.double()[:, torch.arange(Hq) // (Hq // k.shape[1])].gather(2, j)
    lim = torch.where(one, (2.0 ** -8 * D ** -0.5 * (q.double() * kj).abs().sum(dim=-1)).clamp_min(LSE_TOL), torch.full_like(ref, LSE_TOL))
    d = (lse.double() - ref).abs().masked_fill(~live, 0.0)
    fails = [f"lse: |lse - ref| = {float(d[b, h, t]):.3e} >= {float(lim[b, h, t]):.3e} at sample {b}, head {h}, token {t}" for b, h, t in (d >= lim).nonzero().tolist()[:4]]
    return float(d.masked_fill(one, 0.0).max()), float(d.masked_fill(~one, 0.0).max()), fails


def report(label, worst):
    print(f"[attention sweep] {label}: worst block ratio " + "  ".join(f"{n} {w:.3f}" for n, w in worst.items()))
