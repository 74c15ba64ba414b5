"""CPU: the C-ABI of the Tube-Link cross-clip head's prediction-heads training tier -- declared, bound, exported, and its size
functions' limits."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["axvs_tl_heads_train_saved_bytes", "axvs_tl_heads_train_scratch_bytes", "axvs_tl_heads_train_fwd", "axvs_tl_heads_train_bwd"]
#       B, Q, Tc, fpc, h, w, K1, Cm, num_layers
FIXTURES = [(1, 16, 3, 2, 8, 12, 26, 256, 2), (2, 20, 2, 1, 8, 8, 41, 128, 1), (1, 100, 4, 2, 48, 80, 41, 256, 4), (2, 16, 3, 2, 25, 43, 12, 256, 2)]
YTVIS21 = [(1, 100, 3, 3, 128, 228, 41, 256, 4), (1, 100, 3, 3, 96, 168, 41, 256, 4)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from axial_vs_amd import _lib
    return _lib.lib()


def cfg(dims):
    from axial_vs_amd import _lib
    return C.byref(_lib.AxvsTLHeadTrainCfg(*dims))


def test_symbols_declared_bound_and_exported(lib):
    from axial_vs_amd import _lib
    header = open(os.path.join(ROOT, "include", "axvs.h")).read()
    assert "AxvsTLHeadGrads" in header and "AxvsTLHeadTrainCfg" in header
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
    # the gradient struct mirrors the parameter struct field for field
    assert [f[0] for f in _lib.AxvsTLHeadGrads._fields_] == [f[0] for f in _lib.AxvsTLHeadParams._fields_]
    assert C.sizeof(_lib.AxvsTLHeadGrads) == C.sizeof(_lib.AxvsTLHeadParams)


@pytest.mark.parametrize("dims", FIXTURES + YTVIS21)
def test_size_functions(lib, dims):
    assert lib.axvs_tl_heads_train_saved_bytes(cfg(dims)) > 0, dims
    assert 0 < lib.axvs_tl_heads_train_scratch_bytes(cfg(dims), 0) < lib.axvs_tl_heads_train_scratch_bytes(cfg(dims), 1), dims


def test_backward_keeps_no_mask_logits(lib):
    """At the ytvis21 size the saved set is the small per-row activations: far below one layer's mask logits (105 MB)."""
    dims = YTVIS21[0]
    B, Q, Tc, fpc, h, w, K1, Cm, nl = dims
    logits_one_layer = 4 * B * Tc * fpc * Q * h * w
    assert lib.axvs_tl_heads_train_saved_bytes(cfg(dims)) < logits_one_layer // 10


@pytest.mark.parametrize("dims,words", [((1, 10, 3, 3, 8, 8, 41, 256, 4), ["Q=10", "multiple of 4"]),
                                        ((1, 16, 17, 1, 8, 8, 41, 256, 1), ["Tc=17", "16"]),
                                        ((1, 16, 3, 1, 8, 8, 41, 64, 1), ["Cm=64", "128 or 256"]),
                                        ((1, 16, 3, 1, 8, 8, 41, 256, 17), ["num_layers=17", "16"]),
                                        ((1, 16, 3, 1, 16384, 8192, 41, 256, 1), ["h*w=134217728", "67108864"]),
                                        ((0, 16, 3, 1, 8, 8, 41, 256, 1), ["non-positive"])])
def test_out_of_range_configurations_are_refused_with_the_bound(lib, dims, words):
    assert lib.axvs_tl_heads_train_saved_bytes(cfg(dims)) == 0
    msg = lib.axvs_last_error().decode()
    assert all(w in msg for w in words), msg
    assert lib.axvs_tl_heads_train_scratch_bytes(cfg(dims), 1) == 0
