"""CPU: the C-ABI of the deformable encoder layer's training tier -- declared, bound, exported, and its size functions' limits."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["axvs_msda_layer_train_saved_bytes", "axvs_msda_layer_train_scratch_bytes", "axvs_msda_layer_train_fwd",
           "axvs_msda_layer_train_bwd"]
CFG3 = (4, 5376, 256, 8, 3, 4, 1024)       # N, S (64^2 + 32^2 + 16^2), C, heads, levels, points, d_ffn


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from axial_vs_amd import _lib
    return _lib.lib()


def test_symbols_declared_bound_and_exported(lib):
    from axial_vs_amd import _lib
    header = open(os.path.join(ROOT, "include", "axvs.h")).read()
    assert "AxvsMsdaLayerGrads" in header
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None


def test_size_functions(lib):
    for dims in (CFG3, (2, 255, 256, 8, 3, 4, 512), (1, 39, 64, 8, 2, 4, 128), (1, 10, 512, 8, 1, 1, 8)):
        assert lib.axvs_msda_layer_train_saved_bytes(*dims) > 0, dims
        assert 0 < lib.axvs_msda_layer_train_scratch_bytes(*dims, 0) < lib.axvs_msda_layer_train_scratch_bytes(*dims, 1), dims
    # config 3: the activations kept are a few dozen floats per token, far below the HBM of one card
    assert lib.axvs_msda_layer_train_saved_bytes(*CFG3) + lib.axvs_msda_layer_train_scratch_bytes(*CFG3, 1) < 2 ** 30


@pytest.mark.parametrize("dims,words", [((4, 5376, 96, 8, 3, 4, 1024), ["head_dim=12"]),
                                        ((4, 5376, 256, 8, 9, 4, 1024), ["n_levels=9", "8"]),
                                        ((4, 5376, 256, 8, 3, 11, 1024), ["n_levels * n_points = 33", "32"]),
                                        ((1, 100, 256, 4, 1, 1, 1024), ["multiple of 8"]),
                                        ((4, 5376, 256, 8, 3, 4, 1020), ["d_ffn=1020"]),
                                        ((0, 5376, 256, 8, 3, 4, 1024), ["non-positive"])])
def test_out_of_range_dimensions_are_refused_with_the_bound(lib, dims, words):
    assert lib.axvs_msda_layer_train_saved_bytes(*dims) == 0
    msg = lib.axvs_last_error().decode()
    assert all(w in msg for w in words), msg
    assert lib.axvs_msda_layer_train_scratch_bytes(*dims, 1) == 0
