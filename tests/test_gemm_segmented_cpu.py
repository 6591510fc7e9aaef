"""The segmented GEMM entry points without a GPU: the header, the binding table and INTEGRATION.md agree, and the host-side validation returns an error
code -- with a message -- before anything is launched."""

import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mi355_gemm_bf16_segmented", "mi355_gemm_bf16_segmented_tn")
NT, NN, TN = 0, 1, 2
EPI_NONE, EPI_SWIGLU_BWD, EPI_SWIGLU_FWD = 0, 2, 3


def _header():
    text = open(os.path.join(ROOT, "include", "mi355_vlm.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.mark.parametrize("name", NAMES)
def test_header_binding_and_stub_agree(name):
    from llm_quest_amd import _lib

    raw, code = _header()
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
    assert m, f"{name} is not declared in include/mi355_vlm.h"
    args = [a.strip() for a in m.group(1).split(",") if a.strip()]
    assert name in _lib.SIGNATURES and len(args) == len(_lib.SIGNATURES[name])
    for a, t in zip(args, _lib.SIGNATURES[name]):  # pointer / int64 / int, argument by argument
        want = ctypes.c_void_p if "*" in a else ctypes.c_int64 if a.startswith("int64_t") else ctypes.c_int
        assert t is want, (name, a, t)
    # the comment in front of the declaration cites the reference loops it replaces
    comment = raw[: raw.index("int " + name + "(")].rsplit("/*", 1)[1]
    assert "llm_quest/moe/qwen3_moe.py" in raw and ("llm_quest/moe/qwen3_moe.py" in comment or "same two loops" in comment)
    stubs = dict(re.findall(r"_lib\.(mi355_\w+)\.argtypes\s*=\s*\[(.*?)\]", open(os.path.join(ROOT, "INTEGRATION.md")).read()))
    assert name in stubs and len([a for a in stubs[name].split(",") if a.strip()]) == len(args)


@pytest.fixture(scope="module")
def lib():
    from llm_quest_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


@pytest.fixture(scope="module")
def mem():
    buf = ctypes.create_string_buffer(1 << 16)  # host memory: a call that passed validation would fail at the launch, never dereference it here
    return buf, (ctypes.addressof(buf) + 15) // 16 * 16


def _row(lib, p, **over):
    a = dict(form=NT, E=4, counts=p, offsets=p, max_rows=64, R=256, N=64, K=64, A=p, lda=64, B=p, ldb=64, strideB=4096, C=p, ldc=64, residual=None, ldr=0,
             epilogue=EPI_NONE, tile_hint=0)
    a.update(over)
    rc = lib.mi355_gemm_bf16_segmented(*a.values(), None)
    return rc, lib.mi355_last_error().decode()


def _tn(lib, p, **over):
    a = dict(E=4, counts=p, offsets=p, R=256, M=64, N=64, A=p, lda=64, B=p, ldb=64, C=p, ldc=64, strideC=4096, out_dtype=1, residual=None, ldr=0, tile_hint=0)
    a.update(over)
    rc = lib.mi355_gemm_bf16_segmented_tn(*a.values(), None)
    return rc, lib.mi355_last_error().decode()


ROW_REFUSED = {
    "a bad form": (dict(form=7), "form"),
    "the TN form": (dict(form=TN), "form"),
    "E = 129": (dict(E=129), "E must be"),
    "E = 0": (dict(E=0), "E must be"),
    "a null operand": (dict(A=None), "null"),
    "a null table": (dict(counts=None), "null"),
    "lda % 8 != 0": (dict(lda=68), "multiples of 8"),
    "strideB % 8 != 0": (dict(strideB=4100), "multiples of 8"),
    "a misaligned operand": (dict(A="+2"), "aligned"),
    "N % 8 != 0": (dict(N=60), "multiples of 8"),
    "a pitch shorter than the row": (dict(ldc=56), "N columns"),
    "max_rows > R": (dict(max_rows=512), "max_rows"),
    "a tile the kernels do not have": (dict(tile_hint=3), "tile_hint"),
    "an epilogue the kernels do not have": (dict(epilogue=1), "epilogue"),
    "SwiGLU forward on NN": (dict(form=NN, epilogue=EPI_SWIGLU_FWD, residual="p", ldr=64), "SwiGLU forward"),
    "SwiGLU backward on NT": (dict(form=NT, epilogue=EPI_SWIGLU_BWD, residual="p", ldr=128, ldc=128), "SwiGLU backward"),
    "SwiGLU forward without its second output": (dict(epilogue=EPI_SWIGLU_FWD), "SwiGLU forward"),
}


@pytest.mark.parametrize("what", list(ROW_REFUSED))
def test_row_segmented_validation(lib, mem, what):
    _, p = mem
    over, word = ROW_REFUSED[what]
    over = {k: (p if v == "p" else p + 2 if v == "+2" else v) for k, v in over.items()}
    rc, msg = _row(lib, p, **over)
    assert rc != 0 and msg.startswith("mi355_gemm_bf16_segmented") and word in msg, (what, rc, msg)


TN_REFUSED = {
    "E = 129": (dict(E=129), "E must be"),
    "a null operand": (dict(B=None), "null"),
    "ldb % 8 != 0": (dict(ldb=68), "multiples of 8"),
    "M % 8 != 0": (dict(M=60), "multiples of 8"),
    "a bad output dtype": (dict(out_dtype=5), "out_dtype"),
    "experts' outputs that overlap": (dict(strideC=64), "overlap"),
    "a residual pitch shorter than the row": (dict(residual="p", ldr=56), "residual"),
}


@pytest.mark.parametrize("what", list(TN_REFUSED))
def test_k_segmented_validation(lib, mem, what):
    _, p = mem
    over, word = TN_REFUSED[what]
    over = {k: (p if v == "p" else v) for k, v in over.items()}
    rc, msg = _tn(lib, p, **over)
    assert rc != 0 and msg.startswith("mi355_gemm_bf16_segmented_tn") and word in msg, (what, rc, msg)


def test_empty_problems_return_zero_and_valid_ones_reach_the_launch(lib, mem):
    _, p = mem
    assert _row(lib, p, max_rows=0)[0] == 0 and _row(lib, p, R=0, max_rows=0)[0] == 0 and _tn(lib, p, R=0)[0] == 0
    import torch

    if not torch.cuda.is_available():  # a valid call gets as far as the launch, which has no device here: the ABI returns HIP's error like any other
        for rc, msg in (_row(lib, p), _tn(lib, p), _row(lib, p, form=NN, epilogue=EPI_SWIGLU_BWD, residual=p, ldr=128, ldc=128)):
            assert rc == 2 and "launch failed" in msg, (rc, msg)


def test_launchers_check_before_a_pointer_reaches_the_library():
    import torch

    from llm_quest_amd import _lib as L
    from llm_quest_amd import kernels as K

    a = torch.zeros(64, 64, dtype=torch.bfloat16)
    b = torch.zeros(4, 64, 64, dtype=torch.bfloat16)
    t = torch.zeros(5, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.gemm_segmented(L.GEMM_NT, a, b, t[:4], t, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.gemm_segmented_wgrad(a, a, t[:4], t, torch.zeros(4, 64, 64))
    with pytest.raises(RuntimeError, match="uniform stride"):
        K.expert_stack([b[0], b[2], b[1], b[3]])
    with pytest.raises(RuntimeError, match="overlap"):
        K.expert_stack([b[1], b[0]])
    st = K.expert_stack([b[e] for e in range(4)])
    assert tuple(st.shape) == (4, 64, 64) and st.stride() == b.stride() and st.data_ptr() == b.data_ptr()
