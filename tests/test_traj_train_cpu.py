"""CPU: the C-ABI of the full T*H*W layer's training tier -- declared, bound, exported, and its size functions' limits."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["axvs_traj_layer_train_saved_bytes", "axvs_traj_layer_train_scratch_bytes", "axvs_traj_layer_train_fwd",
           "axvs_traj_layer_train_bwd"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from axial_vs_amd import _lib
    return _lib.lib()


def test_symbols_declared_bound_and_exported(lib):
    from axial_vs_amd import _lib
    header = open(os.path.join(ROOT, "include", "axvs.h")).read()
    assert "AxvsTrajLayerGrads" in header
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None


def test_size_functions(lib):
    full = (1, 4, 4096, 256, 8, 1024)                    # [1,4,256,64,64]: 4096 keys per frame, head_dim 32
    assert lib.axvs_traj_layer_train_saved_bytes(*full) > 0
    assert lib.axvs_traj_layer_train_scratch_bytes(*full, 0) > 0
    assert lib.axvs_traj_layer_train_scratch_bytes(*full, 1) > lib.axvs_traj_layer_train_scratch_bytes(*full, 0)
    # no T*HW x HW attention map is kept: activations and scratch of the 64 x 64 layer stay far below its 8.6 GB of logits
    assert lib.axvs_traj_layer_train_saved_bytes(*full) + lib.axvs_traj_layer_train_scratch_bytes(*full, 1) < 2 * 2 ** 30
    assert lib.axvs_traj_layer_train_saved_bytes(1, 17, 64, 256, 8, 1024) == 0
    assert "T=17" in lib.axvs_last_error().decode()
    assert lib.axvs_traj_layer_train_scratch_bytes(1, 2, 400, 256, 4, 1024, 1) == 0      # head_dim 64: a frame must fit in LDS
    msg = lib.axvs_last_error().decode()
    assert "head_dim=64" in msg and "400 keys" in msg and "320" in msg
    assert lib.axvs_traj_layer_train_saved_bytes(1, 2, 320, 256, 4, 1024) > 0
