"""CPU: the test hook into the training tier's split-precision GEMM dispatch (axvs_test_train_gemm) -- declared, bound, exported,
its scratch-size query, and the host-side refusals that return before anything touches the device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["axvs_test_train_gemm_scratch_bytes", "axvs_test_train_gemm"]
ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from axial_vs_amd import _lib
    return _lib.lib()


# host buffers behind the operand pointers: a refused call never reads them, and every call below is refused
_DUMMY = (C.c_float * 64)()


def desc(op, M=128, N=128, K=128, **kw):
    from axial_vs_amd import _lib
    t = _lib.AxvsTestGemm()
    t.op = _lib.TEST_GEMM_OPS[op]
    t.a = t.b = t.c = C.addressof(_DUMMY)
    t.M, t.N, t.K = M, N, K
    t.lda, t.ldb, t.ldc = K, K, N
    t.al_a = t.al_b = t.al_c = 4
    t.mul = t.drop_scale = 1.0
    t.zsplits = 1
    t.variant = -1
    for k, v in kw.items():
        setattr(t, k, C.addressof(_DUMMY) if v is True else v)
    return t


def test_symbols_declared_bound_and_exported(lib):
    from axial_vs_amd import _lib
    header = open(os.path.join(ROOT, "include", "axvs.h")).read()
    assert "test hooks, not part of the drop-in surface" in header and "AxvsTestGemm" in header
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
    # the ctypes mirror lists the header's fields in the header's order
    body = re.search(r"typedef struct AxvsTestGemm \{(.*?)\} AxvsTestGemm;", header, re.S).group(1)
    fields = [n for decl in body.split(";") if decl.strip() for n in re.findall(r"\**\s*(\w+)\s*(?:,|$)", decl.strip())]
    assert fields == [f[0] for f in _lib.AxvsTestGemm._fields_]


def align256(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("N,K", [(136, 72), (8, 8), (24, 40), (1024, 256)])
def test_scratch_bytes(lib, N, K):
    """wgrad: 65 weight-sized partial slots and 64 bias partials; dgrad: the transposed weight; the other forms need none."""
    assert lib.axvs_test_train_gemm_scratch_bytes(C.byref(desc("wgrad", 1000, N, K))) == align256(4 * 65 * N * K) + align256(4 * 64 * N)
    assert lib.axvs_test_train_gemm_scratch_bytes(C.byref(desc("dgrad", 1000, N, K))) == align256(4 * N * K)
    for op in ("nt", "fwd", "tn_direct"):
        assert lib.axvs_test_train_gemm_scratch_bytes(C.byref(desc(op, 1000, N, K))) == 0
    assert lib.axvs_test_train_gemm_scratch_bytes(None) == 0


REFUSALS = [
    # (op, shape / fields, words of axvs_last_error())
    ("nt", dict(N=6), ["N=6", "multiples of 4"]),
    ("nt", dict(ldc=130), ["row strides", "multiples of 4"]),
    ("nt", dict(K=64, lda=66), ["row strides", "multiples of 4"]),          # 16-byte loader (al_a = 4) on a stride of 66 floats
    ("nt", dict(K=64, ldb=70), ["row strides", "multiples of 4"]),
    ("nt", dict(aff=True), ["affine loader", "second operand"]),
    ("fwd", dict(N=130), ["N=130", "multiples of 4"]),
    ("fwd", dict(K=33), ["row strides", "K=33"]),                           # contiguous rows of K floats: the 16-byte loader's rule
    ("dgrad", dict(N=64, K=30), ["N=30", "multiples of 4"]),                # dX = dY W: its width is K
    ("dgrad", dict(N=30, K=64), ["row strides", "multiples of 4"]),         # W^T rows of N floats
    ("wgrad", dict(N=12, K=64), ["N=12", "multiples of 8"]),
    ("wgrad", dict(N=64, K=20), ["K=20", "multiples of 8"]),
    ("wgrad", dict(N=64, K=64, lda=66), ["ldy=66", "multiples of 4"]),      # the weight-gradient kernel only has the 16-byte loader
    ("wgrad", dict(N=64, K=64, ldb=65), ["ldx=65", "multiples of 4"]),
    ("tn_direct", dict(N=6), ["N=6", "multiple of 4"]),
    ("tn_direct", dict(N=64, lda=66), ["multiple of 4"]),
    ("tn_direct", dict(N=256, stat_part=True, stat_rows=128, grp_rows=100, grp_ld=1 << 20), ["grouped output rows", "no statistics"]),
    ("tn_direct", dict(M=1 << 31), ["Mc=2147483648", "2^31"]),
    ("nt", dict(M=0), ["non-positive"]),
    ("wgrad", dict(M=0, N=64, K=64), ["non-positive"]),
    # relu = 2 / 3 (the GELU epilogues): one instantiation, three pieces on the 16-byte loader without a second operand
    ("nt", dict(relu=2, exact=0), ["GELU", "three pieces"]),
    ("nt", dict(relu=2, exact=1, a2=True, aff=True, aff_rows=8), ["GELU", "no second operand"]),
    ("nt", dict(relu=2, exact=1, al_a=2), ["GELU", "16-byte rows"]),
    ("nt", dict(relu=3, exact=1, a2=True), ["GELU", "no second operand"]),
    ("nt", dict(relu=3, exact=1, K=30, lda=32, ldb=32), ["GELU", "K % 4 == 0"]),
    ("nt", dict(relu=2, exact=1, out16=True, kind16=1), ["GELU", "fp32 rows only"]),
    ("fwd", dict(relu=3, exact=0), ["GELU", "three pieces"]),
]


@pytest.mark.parametrize("op,kw,words", REFUSALS, ids=[f"{r[0]}-{'-'.join(r[1])}" for r in REFUSALS])
def test_refusals_return_err_arg_with_the_bound(lib, op, kw, words):
    t = desc(op, **kw)
    assert lib.axvs_test_train_gemm(C.byref(t), C.addressof(_DUMMY), None) == ERR_ARG
    msg = lib.axvs_last_error().decode()
    assert all(w in msg for w in words), msg
    assert t.variant == 0          # nothing was launched


def test_null_pointers_and_unknown_op(lib):
    t = desc("nt")
    t.b = None
    assert lib.axvs_test_train_gemm(C.byref(t), None, None) == ERR_ARG and b"null pointer" in lib.axvs_last_error()
    assert lib.axvs_test_train_gemm(None, None, None) == ERR_ARG
    for op in ("wgrad", "dgrad"):      # these two need their scratch
        assert lib.axvs_test_train_gemm(C.byref(desc(op, 64, 64, 64)), None, None) == ERR_ARG and b"null scratch" in lib.axvs_last_error()
    t = desc("nt")
    t.op = 9
    assert lib.axvs_test_train_gemm(C.byref(t), None, None) == ERR_ARG and b"unknown op 9" in lib.axvs_last_error()
