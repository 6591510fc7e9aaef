"""The kernels at operand sizes whose element / byte offsets pass 2^31 and 2^32 -- where the batch-160 step runs and nothing else in the suite reaches.

Every large operand is built on the device, verified there over its whole extent (exact compares, or fp64 reductions taken chunk by chunk: integers
below 2^53 are exact in fp64) and, on 64-row bands -- the first rows, the band holding the first element offset >= 2^31, the one holding the first
offset >= 2^32, the last ragged rows; positions computed from the shape -- against an integer / fp64 / fp32 reference on the CPU.  Nothing of 1e9
elements or more crosses to the host.  The shapes are the smallest at which an offset can wrap, not the workload's.

Integer operands make the GEMM cases exact: every product and every partial sum is an integer below 2^24, so the fp32 result is defined bit for bit in
any summation order, and a bf16 output is ONE rounding of that exact value.  Each case states its bound and asserts it on the reference.

No case allocates more than 40 GiB; a case skips only when ``torch.cuda.mem_get_info()`` reports less free memory than it needs.

Every test prints its wall time (fixtures included) and its peak ``torch.cuda.max_memory_allocated()`` (run with ``-s``).  Expected from the sizes, NOT YET
MEASURED on a GPU -- replace this table with the printed figures of the first recorded run:

    case                                                   largest live tensors                         peak (computed)
    1  LM-head output, fp32 paths                          2 x fp32 [28 333, 151 936]                   ~33 GiB
    1  LM-head output, bf16 paths / ping-pong (K = 320)    fp32 + bf16 [28 333, 151 936]                ~26 GiB
    2  dgrad / wgrad / grouped / split-K                   bf16 [28 333, 151 936] (or [8.4e6, 512])     ~11 GiB
    3  cross-entropy, in place / out of place              1 or 2 x bf16 [28 333, 151 936]              ~10 / ~18 GiB
    4  attention backward, B = 80 / 129                    dS scratch 2.7e9 / 4.3e9 bytes               ~10 / ~16 GiB
    5  cast, add_f32_to_bf16                               fp32 + bf16 (+ bf16) of 2^32 + 32 792        ~25 / ~33 GiB
    5  scale_bf16, sumsq, clip_scale_                      2 x bf16 / bf16 / fp32 of 2^32 (2^31) + ...  ~17 / ~9 / ~9 GiB
    5  adamw_                                              4 x fp32 of 2^31 + 32 792                    ~35 GiB
"""

import gc
import math
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GIB = 1 << 30
ROWS, VOCAB = 28_333, 151_936  # ROWS * VOCAB = 4 304 802 688 > 2^32; ROWS is ragged against 8, 128 and 256
BAND = 64
CHUNK = 1024  # rows of a [*, VOCAB] operand handled per device pass (an fp64 copy of a chunk is 1.2 GB)
FLAT = 1 << 26  # elements of a flat array handled per device pass
N32 = (1 << 32) + 8 * 4099  # flat sizes: past an unsigned / a signed 32-bit index, with a ragged tail behind the last full 2^k block
N31 = (1 << 31) + 8 * 4099


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from llm_quest_amd import kernels

    return kernels


@pytest.fixture(autouse=True)
def _time_and_peak(request):
    if not torch.cuda.is_available():
        yield
        return
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print(f"\n[large-offsets] {request.node.name}: {time.perf_counter() - t0:.2f} s, peak {torch.cuda.max_memory_allocated() / GIB:.2f} GiB")


def _release():
    gc.collect()
    torch.cuda.empty_cache()


def _need(nbytes):
    """The only skip of this file: less free device memory than the case needs (never more than 40 GiB)."""
    assert nbytes <= 40 * GIB, nbytes
    _release()
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip(f"needs {nbytes} bytes of device memory, torch.cuda.mem_get_info() reports {free} free")


def _row_chunks(rows, step=CHUNK):
    for r0 in range(0, rows, step):
        yield r0, min(r0 + step, rows)


def _band_starts(rows, pitch):
    """First rows of the four bands of an operand with ``rows`` rows of ``pitch`` elements: the first rows, the rows around the one that holds element
    offset 2^31, the rows around the one that holds 2^32, the last rows."""
    assert rows >= 2 * BAND and rows * pitch > 1 << 32
    starts = [0]
    for bit in (31, 32):
        r = (1 << bit) // pitch  # r * pitch <= 2^bit < (r + 1) * pitch: row r holds the first offset >= 2^bit
        assert r < rows
        starts.append(min(max(r - BAND // 2, 0), rows - BAND))
    starts.append(rows - BAND)
    return starts


def _ints_rows(r0, r1, cols, lo, hi, seed, dtype=BF16):
    """Rows r0..r1 of a seeded device matrix of integers in [lo, hi].  A chunk's seed depends on (seed, r0) only, so any chunk of ``_ints_dev`` can be made
    again without keeping a copy of the matrix."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed * 1_000_003 + r0)
    return torch.randint(lo, hi + 1, (r1 - r0, cols), generator=g, device="cuda", dtype=torch.int8).to(dtype)


def _ints_dev(rows, cols, lo, hi, seed, dtype=BF16, step=CHUNK):
    out = torch.empty((rows, cols), dtype=dtype, device="cuda")
    for r0, r1 in _row_chunks(rows, step):
        out[r0:r1] = _ints_rows(r0, r1, cols, lo, hi, seed, dtype)
    return out


def _assert_rows_equal(got, want_rows, what):
    """got[r0:r1] == want_rows(r0, r1) bit for bit, chunk by chunk on the device; names the first wrong row (its position against the tile height and the
    2^31 / 2^32 element offsets points at the 32-bit quantity)."""
    for r0, r1 in _row_chunks(got.shape[0]):
        want = want_rows(r0, r1)
        assert want.dtype == got.dtype and want.shape == got[r0:r1].shape
        if not torch.equal(got[r0:r1], want):
            bad = (got[r0:r1] != want).any(dim=1).nonzero().flatten()
            first = r0 + int(bad[0])
            pytest.fail(f"{what}: first wrong row {first} (element offset {first * got.stride(0)}), {bad.numel()} wrong rows in {r0}..{r1}")


def _rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


# =========================================================================== 1. NT GEMM whose OUTPUT passes 2^32 elements (the LM head)
def _nt_reference(K, a, b):
    """The per-tile kernel (tile hint 2), fp32 output, into a C pre-filled with a sentinel."""
    from llm_quest_amd import _lib as L

    c = torch.full((a.shape[0], b.shape[0]), 777.0, dtype=F32, device="cuda")
    K.gemm(L.GEMM_NT, a, b, out=c, allow_split_k=False, tile=2)
    return c


def _verify_nt_reference(c, a, b):
    """(a) no sentinel left, (b) both checksum identities over the whole matrix, (c) the four row bands against the CPU integer product."""
    M, N, Kd = a.shape[0], b.shape[0], a.shape[1]
    # exactness: operands in {-1, 0, 1}, so every partial sum is an integer of magnitude <= Kd < 2^24: exact in fp32 in any order
    assert Kd < 1 << 24 and int(a.abs().max()) <= 1 and int(b.abs().max()) <= 1
    ai, bi = a.cpu().to(torch.int64), b.cpu().to(torch.int64)  # M x Kd and N x Kd: small
    row_sum = torch.empty(M, dtype=F64, device="cuda")
    col_sum = torch.zeros(N, dtype=F64, device="cuda")
    for r0, r1 in _row_chunks(M):
        blk = c[r0:r1]
        assert not bool((blk == 777.0).any()), f"sentinel left in rows {r0}..{r1}"
        assert float(blk.abs().max()) <= Kd
        row_sum[r0:r1] = blk.sum(dim=1, dtype=F64)
        col_sum += blk.sum(dim=0, dtype=F64)
    # sum_n C[m, n] = A[m, :] . (sum_n B[n, :])   and   sum_m C[m, n] = (sum_m A[m, :]) . B[n, :]; all sums are integers below 2^53
    assert torch.equal(row_sum.cpu().to(torch.int64), ai @ bi.sum(dim=0))
    assert torch.equal(col_sum.cpu().to(torch.int64), bi @ ai.sum(dim=0))
    for r in _band_starts(M, c.stride(0)):
        want = ai[r : r + BAND].double() @ bi.double().t()  # exact: integers far below 2^53
        assert torch.equal(c[r : r + BAND].cpu().double(), want), f"rows {r}..{r + BAND}"


class TestLmHeadOutputPast2p32Elements:
    M, N, KD = ROWS, VOCAB, 128

    @pytest.fixture(scope="class")
    def case(self, K):
        _need(2 * self.M * self.N * 4 + 3 * GIB)  # the reference and one more fp32 output, chunk temporaries
        a = _ints_dev(self.M, self.KD, -1, 1, 11)
        b = _ints_dev(self.N, self.KD, -1, 1, 12)
        case = {"a": a, "b": b, "ref": _nt_reference(K, a, b)}
        yield case
        case.clear()
        _release()

    def test_per_tile_reference_is_exact(self, K, case):
        assert self.M * self.N > 1 << 32 and self.M % 8 and case["ref"].stride(0) == self.N
        _verify_nt_reference(case["ref"], case["a"], case["b"])

    @pytest.mark.parametrize("tile", [1, 3, 4, 5])
    def test_fp32_output_of_every_tile_equals_the_reference(self, K, case, tile):
        from llm_quest_amd import _lib as L

        c = torch.full((self.M, self.N), 777.0, dtype=F32, device="cuda")
        K.gemm(L.GEMM_NT, case["a"], case["b"], out=c, tile=tile)
        ref = case["ref"]
        _assert_rows_equal(c, lambda r0, r1: ref[r0:r1], f"tile {tile}")

    @pytest.mark.parametrize("path", ["library", "walk_off", "per_tile", "pp1", "pp2"])
    def test_bf16_output_equals_the_rounded_reference(self, K, case, path, monkeypatch):
        """bf16 output = one rounding of the exact fp32 value (|C| <= 128: an integer, exact in bf16 even).  ``library``: the persistent kernel with the
        weight-stationary walk (N >= 16 384 column panels' worth); ``walk_off``: the persistent kernel without it; ``per_tile``: the threshold raised so that
        the per-tile kernel takes the launch; ``pp1`` / ``pp2``: the ping-pong switch (with K = 128 < 320 the library keeps such launches on the persistent
        kernel; the ping-pong kernel itself is reached in test_ping_pong_kernel_past_2p32_elements)."""
        from llm_quest_amd import _lib as L

        env = {"library": {}, "walk_off": {"MI355_GEMM_WALK": "0"}, "per_tile": {"MI355_GEMM_PERSIST_MIN_TILES": "1000000000"},
               "pp1": {"MI355_GEMM_PP": "1"}, "pp2": {"MI355_GEMM_PP": "2"}}[path]
        for name in ("MI355_GEMM_WALK", "MI355_GEMM_PERSIST_MIN_TILES", "MI355_GEMM_PP"):
            monkeypatch.delenv(name, raising=False)
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        assert self.KD <= 256  # integers up to 256 are exact in bf16
        ref = case["ref"]
        c = torch.full((self.M, self.N), 776.0, dtype=BF16, device="cuda")  # 776 is a bf16 value no result can take
        K.gemm(L.GEMM_NT, case["a"], case["b"], out=c)
        _assert_rows_equal(c, lambda r0, r1: ref[r0:r1].to(BF16), path)
        if path == "pp2":  # the residual form is the one MI355_GEMM_PP=2 names
            c = _ints_dev(self.M, self.N, -100, 100, 13)
            K.gemm(L.GEMM_NT, case["a"], case["b"], out=c, residual=c)
            _assert_rows_equal(c, lambda r0, r1: (ref[r0:r1] + _ints_rows(r0, r1, self.N, -100, 100, 13, F32)).to(BF16), path + " + residual")

    def test_bf16_accumulate_in_place(self, K, case):
        """out = c, residual = c with integer residuals in [-100, 100]: |sum| <= 228 <= 256, an integer, exact in bf16."""
        from llm_quest_amd import _lib as L

        assert self.KD + 100 <= 256
        ref = case["ref"]
        c = _ints_dev(self.M, self.N, -100, 100, 14)
        K.gemm(L.GEMM_NT, case["a"], case["b"], out=c, residual=c)
        _assert_rows_equal(c, lambda r0, r1: (ref[r0:r1] + _ints_rows(r0, r1, self.N, -100, 100, 14, F32)).to(BF16), "accumulate in place")


@pytest.mark.parametrize("mask", [1, 2])
def test_ping_pong_kernel_past_2p32_elements(K, mask, monkeypatch):
    """``gemm_nt_pp_kernel`` needs K >= 320, so the LM-head case above (K = 128) never reaches it: the same M and N at K = 320.  |C| <= 320 < 2^24 is exact in
    fp32; the bf16 output is one round-to-nearest of that exact value (of value + residual for mask 2, |.| <= 420, exact in fp32 too), which is what ``.to(bfloat16)``
    computes."""
    from llm_quest_amd import _lib as L

    M, N, Kd = ROWS, VOCAB, 320
    _need(M * N * (4 + 2) + 3 * GIB)
    a, b = _ints_dev(M, Kd, -1, 1, 15), _ints_dev(N, Kd, -1, 1, 16)
    ref = _nt_reference(K, a, b)
    _verify_nt_reference(ref, a, b)
    for name in ("MI355_GEMM_WALK", "MI355_GEMM_PERSIST_MIN_TILES"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("MI355_GEMM_PP", str(mask))
    assert Kd + 100 < 1 << 24
    if mask == 1:
        c = torch.full((M, N), 776.0, dtype=BF16, device="cuda")
        K.gemm(L.GEMM_NT, a, b, out=c)
        _assert_rows_equal(c, lambda r0, r1: ref[r0:r1].to(BF16), "ping-pong, plain")
    else:
        c = _ints_dev(M, N, -100, 100, 17)
        K.gemm(L.GEMM_NT, a, b, out=c, residual=c)
        _assert_rows_equal(c, lambda r0, r1: (ref[r0:r1] + _ints_rows(r0, r1, N, -100, 100, 17, F32)).to(BF16), "ping-pong, residual")


# =========================================================================== 2. GEMMs whose INPUT passes 2^32 elements (dgrad / wgrad of the LM head)
class TestLmHeadInputPast2p32Elements:
    M, V, D, DX = ROWS, VOCAB, 256, 128

    @pytest.fixture(scope="class")
    def case(self, K):
        _need(self.M * self.V * 2 + 6 * GIB)
        dl = _ints_dev(self.M, self.V, -1, 1, 21)  # dlogits [tokens, vocabulary]
        w = _ints_dev(self.V, self.D, -1, 1, 22)  # LM-head weight [vocabulary, d]
        x = _ints_dev(self.M, self.DX, -1, 1, 23)  # hidden states [tokens, d'] (the weight gradient's other operand)
        # the checksum identities' right-hand sides, on the device in fp64 (only bands of dlogits go to the host): sums of at most 28 333 * 151 936 integers
        # of magnitude <= 256 stay below 2^53
        wsum, xsum = w.sum(dim=1, dtype=F64), x.sum(dim=1, dtype=F64)
        a_dot_wsum = torch.empty(self.M, dtype=F64, device="cuda")  # A[m, :] . (sum_n W[:, n])
        a_rowsum = torch.empty(self.M, dtype=F64, device="cuda")  # sum_v A[m, v]
        a_colsum = torch.zeros(self.V, dtype=F64, device="cuda")  # sum_m A[m, v]
        at_dot_xsum = torch.zeros(self.V, dtype=F64, device="cuda")  # sum_m A[m, v] * (sum_n X[m, n])
        for r0, r1 in _row_chunks(self.M):
            blk = dl[r0:r1].double()
            a_rowsum[r0:r1] = blk.sum(dim=1)
            a_colsum += blk.sum(dim=0)
            at_dot_xsum += (blk * xsum[r0:r1, None]).sum(dim=0)
            a_dot_wsum[r0:r1] = blk.mul_(wsum).sum(dim=1)
        case = dict(dl=dl, w=w, x=x, a_dot_wsum=a_dot_wsum, a_rowsum=a_rowsum, a_colsum=a_colsum, at_dot_xsum=at_dot_xsum)
        yield case
        case.clear()
        _release()

    @pytest.mark.parametrize("split_k", [False, True])
    def test_nn_dgrad_fp32(self, K, case, split_k):
        """dX = dY W, lda = 151 936: the K loop walks rows of A whose offsets pass 2^32.  A sum has 151 936 terms in {-1, 0, 1}: every partial sum (and every
        split-K slab) is an integer below 2^24, exact in fp32."""
        from llm_quest_amd import _lib as L

        dl, w = case["dl"], case["w"]
        assert self.M * self.V > 1 << 32 and self.V < 1 << 24 and dl.stride(0) == self.V
        c = torch.full((self.M, self.D), 777.0e3, dtype=F32, device="cuda")
        K.gemm(L.GEMM_NN, dl, w, out=c, allow_split_k=split_k)
        assert float(c.abs().max()) <= self.V
        assert torch.equal(c.sum(dim=1, dtype=F64), case["a_dot_wsum"])
        assert torch.equal(c.sum(dim=0, dtype=F64), (case["a_colsum"][:, None] * w.double()).sum(dim=0))
        wc = w.cpu().double()
        for r in _band_starts(self.M, self.V):
            want = dl[r : r + BAND].cpu().double() @ wc  # integers below 2^53: exact
            assert torch.equal(c[r : r + BAND].cpu().double(), want), f"rows {r}..{r + BAND}"

    def test_dgrad_and_nn_bf16_match_the_fp32_result_and_each_other(self, K, case):
        """``K.dgrad`` (W transposed, then NT), the NN form with bf16 output and the persistent NT kernel (tile hint 7; at N = 256 the library's own choice for this
        shape is the 128 x 128 per-tile kernel): each one bf16 rounding of the exact fp32 matrix -- rel_l2 < 3e-3 per band, the suite's bound for one bf16
        rounding of an output -- and, being roundings of the same exact integers, bit-identical to each other."""
        from llm_quest_amd import _lib as L

        dl, w = case["dl"], case["w"]
        c32 = K.gemm(L.GEMM_NN, dl, w, out_dtype=F32, allow_split_k=False)  # verified by test_nn_dgrad_fp32
        assert float(c32.abs().max()) <= self.V < 1 << 24
        nn16 = K.gemm(L.GEMM_NN, dl, w)
        assert K.DGRAD_NT and self.M >= K.DGRAD_NT_MIN_ROWS
        dg = K.dgrad(dl, w)
        persistent = K.gemm(L.GEMM_NT, dl, K.transpose(w), tile=7)
        assert torch.equal(dg, nn16) and torch.equal(persistent, nn16)
        assert torch.equal(nn16, c32.to(BF16))  # one round-to-nearest of an exact value
        for r in _band_starts(self.M, self.V):
            for name, got in (("nn", nn16), ("dgrad", dg), ("persistent", persistent)):
                e = _rel_l2(got[r : r + BAND], c32[r : r + BAND])
                assert e < 3e-3, (name, r, e)

    def _tn_column_bands(self):
        """Bands of OUTPUT rows of dW = dY^T X, which are vocabulary columns of A = dY: the first and the last columns, and the columns in which the walk down A's
        rows first reads an element offset >= 2^31 and >= 2^32."""
        starts = [0]
        for bit in (31, 32):
            starts.append(min(max((1 << bit) % self.V - BAND // 2, 0), self.V - BAND))
        starts.append(self.V - BAND)
        return starts

    @pytest.mark.parametrize("split_k", [False, True])
    def test_tn_wgrad_fp32(self, K, case, split_k):
        """dW = dY^T X with A = dlogits as [K = 28 333 tokens, M = 151 936]: the K loop itself walks A past 2^32 elements.  Sums of 28 333 terms in {-1, 0, 1}:
        exact in fp32."""
        from llm_quest_amd import _lib as L

        dl, x = case["dl"], case["x"]
        assert self.M < 1 << 24
        c = torch.full((self.V, self.DX), 777.0e3, dtype=F32, device="cuda")
        K.gemm(L.GEMM_TN, dl, x, out=c, allow_split_k=split_k)
        assert float(c.abs().max()) <= self.M
        assert torch.equal(c.sum(dim=1, dtype=F64), case["at_dot_xsum"])
        assert torch.equal(c.sum(dim=0, dtype=F64), (case["a_rowsum"][:, None] * x.double()).sum(dim=0))
        xc = x.cpu().double()
        for v in self._tn_column_bands():
            want = dl[:, v : v + BAND].cpu().double().t() @ xc
            assert torch.equal(c[v : v + BAND].cpu().double(), want), f"vocabulary columns {v}..{v + BAND}"

    def test_grouped_tn_equals_the_single_launches(self, K, case):
        from llm_quest_amd import _lib as L

        dl, x = case["dl"], case["x"]
        small = [(_ints_dev(1416, 392, -2, 2, 24), _ints_dev(1416, 264, -2, 2, 25)), (_ints_dev(520, 136, -2, 2, 26), _ints_dev(520, 72, -2, 2, 27))]
        ops = [small[0], (dl, x), small[1]]  # the large problem in the middle: its tiles start behind another problem's
        outs = [torch.full((a.shape[1], b.shape[1]), 777.0e3, dtype=F32, device="cuda") for a, b in ops]
        K.gemm_grouped(L.GEMM_TN, [(a, b, o, None) for (a, b), o in zip(ops, outs)], tile=1)
        for i, ((a, b), o) in enumerate(zip(ops, outs)):
            assert torch.equal(o, K.gemm(L.GEMM_TN, a, b, out_dtype=F32, allow_split_k=False, tile=1)), i
        assert torch.equal(outs[1].sum(dim=1, dtype=F64), case["at_dot_xsum"])


def test_split_k_walks_an_operand_past_2p32_elements(K):
    """At the LM head's shapes above the library never splits K (hundreds of output tiles already fill the chip).  A shape where it does: TN with
    A [2^23 + 4099 tokens, 512] (4.3e9 elements) and B [tokens, 128] -- four 128 x 128 output tiles, so the K loop is cut into slabs and every slab's workgroups start
    their walk at a row offset of their own, the last ones beyond 2^32 elements.  Sums of 8.4e6 terms in {-1, 0, 1} stay below 2^24: exact in fp32, slab by slab.
    Checked against (1) the unsplit kernel, (2) an fp64 product taken chunk by chunk on the device, and (3) the CPU, with A zeroed outside four 64-row bands (first, around
    element offsets 2^31 and 2^32, last), so that the whole result follows from the bands alone."""
    from llm_quest_amd import _lib as L

    tok, M, N = (1 << 23) + 4099, 512, 128
    assert tok * M > 1 << 32 and tok < 1 << 24
    _need(tok * (M + N) * 2 + 6 * GIB)
    a, x = _ints_dev(tok, M, -1, 1, 28, step=1 << 18), _ints_dev(tok, N, -1, 1, 29, step=1 << 18)
    ws = K._workspace(a.device)
    ws.fill_(float("nan"))
    c = K.gemm(L.GEMM_TN, a, x, out_dtype=F32)
    assert bool(torch.isfinite(ws[: 2 * M * N]).all()), "the library did not split K at this shape: the case no longer tests what it is for"
    assert torch.equal(c, K.gemm(L.GEMM_TN, a, x, out_dtype=F32, allow_split_k=False))
    ref = torch.zeros((M, N), dtype=F64, device="cuda")
    for r0, r1 in _row_chunks(tok, 1 << 18):
        ref += a[r0:r1].double().t() @ x[r0:r1].double()  # integers below 2^53: exact
    assert float(ref.abs().max()) < 1 << 24 and torch.equal(c.double(), ref)
    bands = _band_starts(tok, M)
    kept = [(a[r : r + BAND].clone(), x[r : r + BAND].cpu().double()) for r in bands]
    a.zero_()
    want = torch.zeros((M, N), dtype=F64)
    for r, (ab, xb) in zip(bands, kept):
        a[r : r + BAND] = ab
        want += ab.cpu().double().t() @ xb
    ws.fill_(float("nan"))
    c = K.gemm(L.GEMM_TN, a, x, out_dtype=F32)
    assert bool(torch.isfinite(ws[: 2 * M * N]).all())
    assert torch.equal(c.cpu().double(), want)


def test_gemm_refuses_a_leading_dimension_its_31_bit_tile_offsets_cannot_span(K):
    """A tile's DMA offsets are 31-bit, relative to a 64-bit tile origin: 256 rows of an operand must span less than 2 GiB.  A row pitch of 2^22 elements is the first
    that does not -- refused, not computed with a wrapped offset; eight elements less is served, and exactly."""
    from llm_quest_amd import _lib as L

    rows, Kd, limit = 8, 64, (1 << 31) // 512  # lda * 2 bytes * 256 rows < 2^31
    store = torch.zeros((rows - 1) * limit + Kd, dtype=BF16, device="cuda")
    b = _ints_dev(128, Kd, -2, 2, 61)
    vals = _ints_dev(rows, Kd, -2, 2, 62)
    with pytest.raises(RuntimeError, match="leading dimension"):
        K.gemm(L.GEMM_NT, store.as_strided((rows, Kd), (limit, 1)), b, out_dtype=F32)
    with pytest.raises(RuntimeError, match="leading dimension"):
        K.gemm(L.GEMM_NN, _ints_dev(128, rows, -2, 2, 63), store.as_strided((rows, Kd), (limit, 1)), out_dtype=F32)  # the same for ldb
    a = store.as_strided((rows, Kd), (limit - 8, 1))
    a.copy_(vals)
    assert torch.equal(K.gemm(L.GEMM_NT, a, b, out_dtype=F32), K.gemm(L.GEMM_NT, vals, b, out_dtype=F32))
    assert torch.equal(K.gemm(L.GEMM_NT, a, b, out_dtype=F32).cpu().double(), vals.cpu().double() @ b.cpu().double().t())


# =========================================================================== 3. cross-entropy over more than 2^32 logits
def _logit_rows(r0, r1, V, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed * 1_000_003 + r0)
    return (torch.randn((r1 - r0, V), generator=g, device="cuda") * 3).to(BF16)


@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("rows,V", [(ROWS, VOCAB), (27_700, 155_656)])
def test_cross_entropy_past_2p32_logits(K, rows, V, inplace):
    """V = 151 936: the row-in-registers kernel with 19 chunks per thread; V = 155 656: the two-read kernel.  A block walks rows blockIdx.x, + 65 535, ...; a row's
    base is row * ldl."""
    assert rows * V > 1 << 32 and V % 8 == 0
    _need((2 if inplace else 3) * rows * V * 2 + 4 * GIB)
    seed, scale = 31 + V, 0.125
    x = torch.empty((rows, V), dtype=BF16, device="cuda")
    for r0, r1 in _row_chunks(rows):
        x[r0:r1] = _logit_rows(r0, r1, V, seed)
    bands = _band_starts(rows, V)
    tg = torch.randint(0, V, (rows,), generator=torch.Generator().manual_seed(seed))
    last = bands[-1]
    tg[last + 3], tg[last + 7], tg[last + 11], tg[last + 13] = -100, V + 5, 0, V - 1  # ignored, out of range, first / last element: all inside the last band
    for r in bands[:-1]:
        tg[r + 5] = -100
    ignored, out_of_range = (tg == -100).nonzero().flatten(), (tg == V + 5).nonzero().flatten()
    valid = (tg >= 0) & (tg < V)
    band_logits = [x[r : r + BAND].cpu() for r in bands]  # before the kernel runs: in place it overwrites them
    loss, dl = K.cross_entropy(x, tg.cuda(), want_grad=True, grad_scale=torch.tensor([scale], dtype=F32, device="cuda"), inplace=inplace)
    assert (dl.data_ptr() == x.data_ptr()) == inplace
    # the four bands against fp32 torch on the CPU: loss rows to 1e-5, gradient to 4e-3 (the bounds of test_cross_entropy_forms_agree_with_fp32)
    loss_c = loss.cpu()
    for r, lg in zip(bands, band_logits):
        ok = valid[r : r + BAND].nonzero().flatten()
        lref = lg.float().requires_grad_(True)
        ref = torch.nn.functional.cross_entropy(lref[ok], tg[r : r + BAND][ok], reduction="none")
        ref.sum().backward()
        err = float((loss_c[r : r + BAND][ok] - ref.detach()).abs().max())
        assert err < 1e-5 * float(ref.detach().abs().max()), (r, err)
        e = _rel_l2(dl[r : r + BAND].cpu()[ok], lref.grad[ok] * scale)
        assert e < 4e-3, (r, e)
    # all rows, on the device
    assert bool(torch.isfinite(loss[valid.cuda()]).all())
    assert bool((loss_c[ignored] == 0).all()) and bool(torch.isnan(loss_c[out_of_range]).all()) and ignored.numel() == 4 and out_of_range.numel() == 1
    assert int(torch.count_nonzero(dl[torch.cat((ignored, out_of_range)).cuda()])) == 0  # rows of ignored (and refused) targets: exactly zero
    # Every gradient row sums to 0 in exact arithmetic (softmax sums to 1, minus the one-hot).  What is stored are V terms, each below grad_scale in magnitude and
    # each rounded to bf16, i.e. off by at most 2^-8 of itself; V such errors of independent sign add up to at most grad_scale * 2^-8 * sqrt(V).  (The hard bound,
    # 2^-9 * sum |g_i| <= grad_scale * 2^-8, is smaller still; the fp32 softmax's own error, ~V * 2^-24 relative, is far below either.)
    bound = scale * 2.0**-8 * math.sqrt(V)
    for r0, r1 in _row_chunks(rows):
        s = dl[r0:r1].sum(dim=1, dtype=F64).abs()
        assert float(s.max()) <= bound, (r0 + int(s.argmax()), float(s.max()), bound)
    if not inplace:
        _assert_rows_equal(x, lambda r0, r1: _logit_rows(r0, r1, V, seed), "logits after the out-of-place call")


# =========================================================================== 4. attention backward with a dS scratch above 2^31 / 2^32 bytes
def _per_group_rel(a, b, B, S, Hkv):
    """rel_l2 of every (batch, kv-head) group's slice of a [B*S, Hkv * w] gradient: one misaddressed (batch, head) pair cannot hide in the whole tensor's norm."""
    a4, b4 = a.view(B, S, Hkv, -1).double(), b.view(B, S, Hkv, -1).double()
    return (a4 - b4).pow(2).sum(dim=(1, 3)).sqrt() / (b4.pow(2).sum(dim=(1, 3)).sqrt() + 1e-30)


@pytest.mark.parametrize("B,boundary_bits", [(80, (31,)), (129, (31, 32))])
def test_attention_backward_scratch_past_2p31_and_2p32_bytes(K, monkeypatch, B, boundary_bits):
    """S = 1024, D = 128, causal, Hq = 16, Hkv = 8: at least 512 (batch, head) pairs, so the persistent backward runs.  B = 80: 2.68e9 bytes of dS, under the default
    4 GiB cap; B = 129: 4.33e9 bytes, with the cap raised.  (i) the scratch form against the recompute form per (batch, kv-head) group at the suite's 6e-3;
    (ii) against fp64 (4e-3 forward, 8e-3 gradients, as test_attention_fwd_bwd) for the first group, the last, and the groups whose dS block holds byte 2^31 / 2^32."""
    from test_kernels_gpu import _attn_ref

    from llm_quest_amd import _lib as L

    S, D, Hq, Hkv = 1024, 128, 16, 8
    G = Hq // Hkv
    lib = L.load()
    need = lib.mi355_attn_bwd_workspace_bytes(B, S, Hq, D)
    ds_bytes = lib.mi355_attn_bwd_workspace_rowconst_offset(B, S, Hq, D, 0)  # the dS blocks come first, the row constants behind them
    assert B * Hkv >= 512 and 0 < ds_bytes < need and ds_bytes > 1 << max(boundary_bits)
    per_head = ds_bytes // (B * Hq)  # bytes of one (batch, query head) block; blocks are laid out in (batch, head) order
    assert per_head * B * Hq == ds_bytes
    _need(4 * need + 6 * GIB)  # the launcher takes the scratch only when it is under a quarter of the free memory
    default_cap = 4096 << 20
    assert (need > default_cap) == (32 in boundary_bits)
    monkeypatch.setattr(K, "_ATTN_DS_SPILL_MAX", max(default_cap, need))
    K.release_attention_scratch()
    try:
        g = torch.Generator(device="cuda")
        g.manual_seed(40 + B)
        q, k, v, do = (torch.randn((B * S, w * D), generator=g, device="cuda").to(BF16) for w in (Hq, Hkv, Hkv, Hq))
        o, lse = K.attn_fwd(q, k, v, B, S, Hq, Hkv, D, causal=True)
        grads = {}
        for form in ("spill", "recompute"):
            monkeypatch.setattr(K, "_ATTN_DS_SPILL", form == "spill")
            before = dict(K.attn_bwd_form)
            dq, dk, dv = (torch.full_like(t, float("nan")) for t in (q, k, v))
            K.attn_bwd(q, k, v, o, do, lse, B, S, Hq, Hkv, D, dq, dk, dv, causal=True)
            assert K.attn_bwd_form[form] == before[form] + 1, (form, before, K.attn_bwd_form)
            grads[form] = (dq, dk, dv)
        assert max(ws.numel() for ws in K._ATTN_WS.values()) >= need
        for name, a, b in zip(("dq", "dk", "dv"), grads["spill"], grads["recompute"]):
            assert bool(torch.isfinite(a.float()).all()) and bool(torch.isfinite(b.float()).all()), name
            rel = _per_group_rel(a, b, B, S, Hkv)
            worst = int(rel.argmax())
            assert float(rel.max()) < 6e-3, (name, divmod(worst, Hkv), float(rel.max()))
        groups = {(0, 0), (B - 1, Hkv - 1)}
        for bit in boundary_bits:
            b_, hq = divmod((1 << bit) // per_head, Hq)  # the block that holds byte offset 2^bit
            assert b_ < B
            groups.add((b_, hq // G))
        dq, dk, dv = grads["spill"]
        for b_, h in sorted(groups):
            rows, qc, kc = slice(b_ * S, (b_ + 1) * S), slice(h * G * D, (h + 1) * G * D), slice(h * D, (h + 1) * D)
            qr, kr, vr = (t.double().requires_grad_(True) for t in (q[rows, qc], k[rows, kc], v[rows, kc]))
            o_ref, _ = _attn_ref(qr, kr, vr, 1, S, G, 1, D, None, True)  # fp64, on the device, this group alone
            o_ref.backward(do[rows, qc].double())
            e = _rel_l2(o[rows, qc], o_ref.detach())
            assert e < 4e-3, ("o", b_, h, e)
            for name, got, ref in (("dq", dq[rows, qc], qr.grad), ("dk", dk[rows, kc], kr.grad), ("dv", dv[rows, kc], vr.grad)):
                e = _rel_l2(got, ref)
                assert e < 8e-3, (name, b_, h, e)
    finally:
        K.release_attention_scratch()


# =========================================================================== 5. flat kernels with n above 2^31 and above 2^32
def _pattern(i0, i1, shift=0):
    """(i + shift) % 251 - 125 for i in [i0, i1): 251 is prime, so an index that lost a high bit (2^31 % 251 = 171, 2^32 % 251 = 91) reads another value."""
    return (torch.arange(i0 + shift, i1 + shift, dtype=torch.int64, device="cuda") % 251 - 125).to(F32)


def _flat_chunks(n, step=FLAT):
    for i0 in range(0, n, step):
        yield i0, min(i0 + step, n)


def _fill(n, dtype, value):
    out = torch.empty(n, dtype=dtype, device="cuda")
    for i0, i1 in _flat_chunks(n):
        out[i0:i1] = value(i0, i1)
    return out


def _bf16_ulp_distance(a, b):
    def ordered(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)

    return int((ordered(a) - ordered(b)).abs().max())


def test_cast_past_2p32_elements(K):
    """fp32 -> bf16 and back, bit-exact against torch's own casts over the whole array."""
    n = N32
    _need(n * (4 + 2) + 3 * GIB)
    src = _fill(n, F32, lambda i0, i1: _pattern(i0, i1) * 0.37)  # (no multiple of a bf16 step: the rounding is exercised too)
    xb = K.cast(src, BF16)
    for i0, i1 in _flat_chunks(n):
        assert torch.equal(xb[i0:i1], src[i0:i1].to(BF16)), (i0, i1)
    del src
    _release()
    xf = K.cast(xb, F32)
    for i0, i1 in _flat_chunks(n):
        assert torch.equal(xf[i0:i1], xb[i0:i1].float()), (i0, i1)


def test_scale_bf16_past_2p32_elements(K):
    n = N32
    _need(n * (2 + 2) + 3 * GIB)
    x = _fill(n, BF16, lambda i0, i1: _pattern(i0, i1).to(BF16))
    y = K.scale_bf16(x, torch.tensor([0.37], dtype=F32, device="cuda"))
    for i0, i1 in _flat_chunks(n):
        assert _bf16_ulp_distance(y[i0:i1], (x[i0:i1].float() * 0.37).to(BF16)) <= 1, (i0, i1)


def test_add_f32_to_bf16_past_2p32_elements(K):
    n = N32
    _need(n * (4 + 2 + 2) + 3 * GIB)
    a = _fill(n, F32, lambda i0, i1: _pattern(i0, i1) * 0.37)
    b = _fill(n, BF16, lambda i0, i1: _pattern(i0, i1, 17).to(BF16))
    d = torch.empty(n, dtype=BF16, device="cuda")
    K.add_f32_to_bf16(a, b, d)
    for i0, i1 in _flat_chunks(n):
        assert _bf16_ulp_distance(d[i0:i1], (a[i0:i1] + b[i0:i1].float()).to(BF16)) <= 1, (i0, i1)


def test_sumsq_past_2p32_elements(K):
    """The full pattern to the suite's bound for this kernel (1e-4 of the fp64 sum, test_cast_clip_helpers) -- and, because a tail of 8 * 4099 elements is only 8e-6
    of that sum, the same array zeroed except for windows at 2^31, at 2^32 and at the very end: there the sum of squares is an integer below 2^24, every partial sum
    is exact in fp32, and the result must EQUAL it."""
    n = N32
    _need(n * 2 + 3 * GIB)
    x = _fill(n, BF16, lambda i0, i1: _pattern(i0, i1).to(BF16))
    ref = sum(float(x[i0:i1].double().pow(2).sum()) for i0, i1 in _flat_chunks(n))
    acc = torch.zeros(1, dtype=F32, device="cuda")
    K.sumsq_into(x, acc)
    assert abs(float(acc) - ref) < 1e-4 * ref, (float(acc), ref)
    windows = [(0, 300), ((1 << 31) - 150, (1 << 31) + 150), ((1 << 32) - 150, (1 << 32) + 150), (n - 300, n)]
    kept = [x[i0:i1].clone() for i0, i1 in windows]
    x.zero_()
    exact = 0.0
    for (i0, i1), w in zip(windows, kept):
        x[i0:i1] = w
        exact += float(w.double().pow(2).sum())
    assert 0 < exact < 1 << 24
    acc.zero_()
    K.sumsq_into(x, acc)
    assert float(acc) == exact, (float(acc), exact)
    x[n - 300 :] = 0  # without the tail behind 2^32 the sum must drop by exactly that window's squares
    acc.zero_()
    K.sumsq_into(x, acc)
    assert float(acc) == exact - float(kept[-1].double().pow(2).sum())


def test_clip_scale_past_2p31_elements(K):
    """x *= min(1, max_norm / (sqrt(sumsq) + 1e-6)) in fp32.  Bound per element: the coefficient is one square root, one addition and one division in fp32 and the
    product one more rounding -- a few units of 2^-24; 2^-21 of the fp64 value leaves room for a square root / division that is not correctly rounded, and is five
    orders of magnitude below what a wrong index gives."""
    n = N31
    _need(n * 4 + 3 * GIB)
    x = _fill(n, F32, lambda i0, i1: _pattern(i0, i1) * 0.37)
    K.clip_scale_(x, torch.tensor([16.0], dtype=F32, device="cuda"), 1.0)
    coef = 1.0 / (4.0 + 1e-6)
    for i0, i1 in _flat_chunks(n):
        want = (_pattern(i0, i1) * 0.37).double() * coef
        err = (x[i0:i1].double() - want).abs()
        assert bool((err <= 2.0**-21 * want.abs()).all()), (i0, i1, float(err.max()))


_ADAMW = dict(step=3, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1)


def _adamw_inputs(i0, i1):
    """Parameter, gradient and both moments as functions of the index (fp32, as stored)."""
    return _pattern(i0, i1), _pattern(i0, i1, 7) / 128, _pattern(i0, i1, 13) / 256, (_pattern(i0, i1, 29) / 128).square()


def _adamw_check(outs, i0, i1, device):
    """Elements [i0, i1) of the updated (param, exp_avg, exp_avg_sq) against the closed-form fp64 update, evaluated on ``device``."""
    p, g, m, v = (t.to(device).double() for t in _adamw_inputs(i0, i1))
    f32 = lambda x: torch.tensor(x, dtype=F32)
    # the hyper-parameters as the kernel receives them: fp32 betas, and 1 - beta taken in fp32 (1 - 0.999f is 4.7e-5 off 0.001: a property of the ABI, not an error)
    b1, b2 = (float(f32(b)) for b in _ADAMW["betas"])
    omb1, omb2 = (float(f32(1.0) - f32(b)) for b in _ADAMW["betas"])
    t, lr, eps, wd = _ADAMW["step"], float(f32(_ADAMW["lr"])), float(f32(_ADAMW["eps"])), float(f32(_ADAMW["weight_decay"]))
    m1 = b1 * m + omb1 * g
    v1 = b2 * v + omb2 * g * g
    den = v1.sqrt() / math.sqrt(1 - b2**t) + eps
    upd = (lr / (1 - b1**t)) * m1 / den
    want = p * (1 - lr * wd) - upd
    got_p, got_m, got_v = (o[i0:i1].to(device).double() for o in outs)
    # the parameter: the bound tests/test_models_gpu.py uses for ArenaAdamW against torch.optim.AdamW ...
    err = (got_p - want).abs()
    assert float(err.max()) <= 2**-7 * float(want.abs().max()) + 1e-6, (i0, i1, float(err.max()))
    # ... which an element that was never updated would still meet, so also element by element, from the fp32 arithmetic: the decay product and the subtraction
    # round at 2^-24 of |p| each; the update carries the bias correction 1 - beta2^t = 3e-3, which loses 2^-24 / 3e-3 = 2e-5 to cancellation in fp32 (1e-4 asserted),
    # and the rounding of the two terms of the first moment (see below) through the same quotient
    m_terms = (b1 * m).abs() + (omb1 * g).abs()
    tol = 2.0**-20 * p.abs() + 1e-4 * upd.abs() + 2.0**-20 * (lr / (1 - b1**t)) * m_terms / den + 1e-7
    assert bool((err <= tol).all()), (i0, i1, float((err / tol).max()))
    # the moments: two fp32 products and one addition each, i.e. at most 3 * 2^-24 of the larger term; 2^-21 of the terms' magnitudes is asserted
    assert bool(((got_m - m1).abs() <= 2.0**-21 * m_terms).all()), (i0, i1)
    assert bool(((got_v - v1).abs() <= 2.0**-21 * v1).all()), (i0, i1)


def test_adamw_past_2p31_elements(K):
    """Four fp32 arrays of 2^31 + 8 * 4099 elements (34 GB).  The closed-form fp64 update on the first and the last 2^16 elements and on 2^16 elements astride index 2^31,
    on the CPU; then the same formula over the whole array, chunk by chunk on the device (the inputs are functions of the index, so no copy of them is kept)."""
    n = N31
    _need(4 * n * 4 + 4 * GIB)
    p, g, m, v = (_fill(n, F32, lambda i0, i1, j=j: _adamw_inputs(i0, i1)[j]) for j in range(4))
    K.adamw_(p, g, m, v, **_ADAMW)
    w = 1 << 16
    for i0 in (0, (1 << 31) - w // 2, n - w):
        _adamw_check((p, m, v), i0, i0 + w, "cpu")
    for i0, i1 in _flat_chunks(n, 1 << 24):
        _adamw_check((p, m, v), i0, i1, "cuda")
    for i0, i1 in _flat_chunks(n):  # the gradient is an input: untouched
        assert torch.equal(g[i0:i1], _adamw_inputs(i0, i1)[1]), (i0, i1)
