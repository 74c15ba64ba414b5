"""CPU: the restatement of the ConvNeXt / ConvNeXtV2 backbone (tests/convnext_cases.py) against fixtures of the reference's own classes,
the modules' state-dict names and shapes, their refusals, the new C-ABI symbols (axvs_cnx_*) and their argument errors, which are
reported before any device work -- and that the cases can tell a wrong halo, a wrong pad rule, shared GRN statistics and (the cases at
ConvNeXt-L's widths) a contraction one k-step short apart."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import convnext_cases as cc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SYMBOLS = ["axvs_cnx_packed_bytes", "axvs_cnx_pack", "axvs_cnx_workspace_bytes", "axvs_cnx_fwd", "axvs_cnx_stem_fwd", "axvs_cnx_down_fwd",
           "axvs_cnx_dwln_fwd", "axvs_cnx_block_fwd"]


@pytest.fixture(scope="session", autouse=True)
def built():
    ge.build()


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    m = json.loads(bytes(z["meta"]).decode())
    case = cc.Net(m["name"], m["seed"], tuple(m["size"]), m["N"], tuple(m["dims"]), tuple(m["depths"]), m["v2"], m["gamma"])
    return case, m, z


def make_module(case, device=None, **kw):
    import axial_vs_amd as ax
    ctx = torch.device(device) if device else torch.device("cpu")
    with ctx:
        if case.v2:
            return ax.ConvNeXtV2Backbone(depths=case.depths, dims=case.dims, **kw)
        return ax.ConvNeXtBackbone(depths=case.depths, dims=case.dims, layer_scale_init_value=1e-6 if case.gamma else 0.0, **kw)


@pytest.mark.parametrize("fx", [c.name for c in cc.FIXTURES])
def test_restatement_equals_the_reference_bit_for_bit(fx):
    """The reference's own eval forward (fp32, CPU) against the float32 restatement on the same weights and input: the same ops in the
    same order, so the same bits -- on a CPU whose float32 kernels are the generator's.  torch's CPU kernels differ between processors
    (measured: on the MI355X machine's host the stem already differs in the last bits from a fixture written on the build machine), so
    equal bits are asserted where this CPU's fingerprint (convnext_cases.cpu_probe, independent of the restatement) is the one the fixture
    records, and on every machine each output lies within 8 x the float32 restatement's own error against float64 of the reference's run
    (the standing bound for a restatement against its reference).  The key list is the fixture's, in the reference's order."""
    case, m, z = load_fixture(fx)
    assert case == next(c for c in cc.FIXTURES if c.name == fx)
    assert m["keys"] == list(cc.param_shapes(case.dims, case.depths, case.v2))
    st = cc.study(case)
    same_cpu = cc.cpu_probe() == m["probe"]
    for k in cc.OUTPUTS:
        ref = torch.from_numpy(z[k])
        e, own = cc.err(st["f32"][k], ref), st["tol"][k] / 8
        print(f"{fx} {k}: float32 restatement against the reference's fp32 run {e:.3e} (own error against float64 {own:.3e}); generator's CPU arithmetic: {same_cpu}")
        assert e <= 8 * own, k
        if same_cpu:
            assert torch.equal(st["f32"][k], ref), k
    assert os.path.getsize(os.path.join(GOLDEN, fx + ".npz")) < 256 * 1024


def test_the_reference_order_needs_float32_weights():
    """Why the yardstick is a restatement: the reference's LayerNorm casts its input to float, and F.layer_norm then meets float values
    and double weights."""
    with pytest.raises(RuntimeError):
        torch.nn.functional.layer_norm(torch.randn(2, 4, dtype=torch.float64).float(), (4,), torch.ones(4, dtype=torch.float64), None, 1e-6)


@pytest.mark.parametrize("v2", [False, True], ids=["v1", "v2"])
def test_large_configuration_names_and_shapes(v2):
    """ConvNeXt-L / ConvNeXtV2-L on the meta device: 340 / 376 entries under the reference's names, in its order, with its shapes"""
    case = cc.Net("L", 0, (1, 1), 1, **cc.LARGE, v2=v2, gamma=True)
    mod = make_module(case, "meta")
    want = cc.param_shapes(case.dims, case.depths, v2)
    sd = mod.state_dict()
    assert len(sd) == (376 if v2 else 340)
    assert list(sd) == list(want)
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(want)
    assert tuple(sd["stages.2.26.pwconv1.weight"].shape) == (3072, 768)
    if v2:
        assert tuple(sd["stages.3.2.grn.gamma"].shape) == (1, 1, 1, 6144)
    assert sum(p.numel() for p in mod.parameters()) == sum(int(np.prod(s)) for s in want.values())


@pytest.mark.parametrize("fx", [c.name for c in cc.FIXTURES])
def test_state_dict_loads_strictly(fx):
    case, m, _ = load_fixture(fx)
    mod = make_module(case)
    assert list(mod.state_dict()) == m["keys"]
    ck = cc.net_params(case)
    mod.load_state_dict(ck, strict=True)
    assert torch.equal(mod.state_dict()["stages.2.1.pwconv2.weight"], ck["stages.2.1.pwconv2.weight"])


def test_no_gamma_configuration():
    import axial_vs_amd as ax
    mod = ax.ConvNeXtBackbone(depths=(1, 1, 1, 1), dims=(16, 16, 16, 16), layer_scale_init_value=0.0)
    assert not any(k.endswith("gamma") for k in mod.state_dict())
    assert list(mod.state_dict()) == list(cc.param_shapes((16,) * 4, (1,) * 4, False, gamma=False))


def test_output_shape_and_size_divisibility():
    import axial_vs_amd as ax
    mod = ax.ConvNeXtV2Backbone(depths=(1, 1, 1, 1), dims=(16, 32, 48, 64), out_features=("stem", "res3", "res5"))
    shp = mod.output_shape()
    assert list(shp) == ["stem", "res3", "res5"]
    assert [(s.channels, s.stride) for s in shp.values()] == [(16, 2), (32, 8), (64, 32)]       # (the reference's table lists the stem at 2)
    assert mod.size_divisibility == -1 and mod.num_features == [16, 32, 48, 64]
    from axial_vs_amd.convnext import map_sizes
    assert map_sizes(769, 1345) == [(193, 337), (97, 169), (49, 85), (25, 43)] == cc.map_sizes(769, 1345)


@pytest.mark.parametrize("kw, text", [(dict(in_chans=4), "in_chans = 3"), (dict(dims=(16, 32, 64, 120)), "multiples of 16 in 16..2048"),
                                      (dict(dims=(16, 32, 64, 4096)), "multiples of 16 in 16..2048"), (dict(dims=(8, 32, 64, 128)), "16..2048"),
                                      (dict(depths=(1, 1, 1), dims=(16, 32, 64)), "four stages"), (dict(depths=(1, 1, 65, 1)), "1..64 blocks"),
                                      (dict(depths=(1, 0, 1, 1)), "1..64 blocks")])
@pytest.mark.parametrize("v2", [False, True], ids=["v1", "v2"])
def test_refusals_at_construction(kw, text, v2):
    import axial_vs_amd as ax
    args = dict(depths=(1, 1, 1, 1), dims=(16, 32, 64, 128))
    args.update(kw)
    with torch.device("meta"), pytest.raises(NotImplementedError, match=text):
        (ax.ConvNeXtV2Backbone if v2 else ax.ConvNeXtBackbone)(**args)


@pytest.mark.parametrize("v2", [False, True], ids=["v1", "v2"])
def test_train_mode_and_cpu_tensors_raise(v2):
    mod = make_module(cc.Net("t", 0, (8, 8), 1, (16, 16, 16, 16), (1, 1, 1, 1), v2, True))
    assert mod.training
    with pytest.raises(NotImplementedError, match="eval"):
        mod(torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mod.eval()(torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError, match=r"\(N, 3, H, W\)"):
        mod(torch.zeros(1, 4, 8, 8))


def _cfg(**kw):
    from axial_vs_amd import _lib
    i4 = ctypes.c_int * 4
    f = dict(N=1, H=9, W=9, dims=(16, 32, 64, 128), depths=(1, 1, 1, 1), h=(3, 2, 1, 1), w=(3, 2, 1, 1), v2=0)
    f.update(kw)
    return _lib.AxvsCnxCfg(N=f["N"], H=f["H"], W=f["W"], dims=i4(*f["dims"]), depths=i4(*f["depths"]), h=i4(*f["h"]), w=i4(*f["w"]), v2=f["v2"])


def test_symbols_and_size_queries():
    from axial_vs_amd import _lib
    L = _lib.lib()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(raw, s) and s in _lib.SIGNATURES, s
    from axial_vs_amd import _params as P
    v1, v2 = _cfg(), _cfg(v2=1)
    for cfg, is_v2 in ((v1, False), (v2, True)):
        slots = [s for i in range(4) for s in P.convnext_down_shapes((16, 32, 64, 128), i)]
        slots += [s for d in (16, 32, 64, 128) for s in P.convnext_block_shapes(d, is_v2)]
        want = sum((4 * int(np.prod(shape)) + 255) // 256 * 256 for _, shape in slots if shape is not None)
        assert L.axvs_cnx_packed_bytes(ctypes.byref(cfg)) == want
    assert L.axvs_cnx_workspace_bytes(ctypes.byref(v2)) > L.axvs_cnx_workspace_bytes(ctypes.byref(v1)) > 0
    assert [n for n, _ in P.convnext_down_shapes((16,) * 4, 1)] == list(_lib.CNX_DOWN_FIELDS)
    assert [n for n, _ in P.convnext_block_shapes(16, True)] == list(_lib.CNX_BLOCK_FIELDS)
    # the large configuration: 196 M parameters + GRN, 4 bytes each
    big = _cfg(**cc.LARGE)
    assert 780e6 < L.axvs_cnx_packed_bytes(ctypes.byref(big)) < 800e6


def test_folded_parameters_have_the_stated_shapes():
    from axial_vs_amd import _params as P
    for v2 in (False, True):
        dims = (16, 32, 64, 128)
        sd = cc.draw(cc.param_shapes(dims, (1, 1, 1, 1), v2), 5)
        for i in range(4):
            got = P.convnext_down_folded(sd, i)
            assert [tuple(t.shape) for t in got] == [s for _, s in P.convnext_down_shapes(dims, i)]
            got = P.convnext_block_folded(sd, f"stages.{i}.0.")
            assert [None if t is None else tuple(t.shape) for t in got] == [s for _, s in P.convnext_block_shapes(dims[i], v2)]
            assert all(t is None or t.dtype == torch.float64 for t in got)
    # the downsample weight in patch order (ky, kx, c)
    w = P.convnext_down_folded(sd, 1)[2]
    assert float(w[3, (1 * 2 + 0) * 16 + 5]) == float(sd["downsample_layers.1.1.weight"][3, 5, 1, 0])
    # v1: gamma folded into pwconv2
    sd = cc.draw(cc.param_shapes(dims, (1, 1, 1, 1), False), 6)
    got = P.convnext_block_folded(sd, "stages.0.0.")
    assert torch.equal(got[6], sd["stages.0.0.pwconv2.weight"].double() * sd["stages.0.0.gamma"].double()[:, None])
    assert float(got[0][3 * 7 + 2, 5]) == float(sd["stages.0.0.dwconv.weight"][5, 0, 3, 2])


def test_folding_calls_no_matrix_product():
    """The fold runs on the parameters' device.  torch's first matrix product on a GPU allocates its BLAS workspace (128 MiB that stay
    allocated for the process, and in the way of every later test that measures peak memory), so `W2 beta` is a product and a row sum."""
    from torch.overrides import TorchFunctionMode
    from axial_vs_amd import _params as P
    seen = []

    class Record(TorchFunctionMode):
        def __torch_function__(self, func, types, args=(), kwargs=None):
            seen.append(getattr(func, "__name__", str(func)))
            return func(*args, **(kwargs or {}))
    for v2 in (False, True):
        sd = cc.draw(cc.param_shapes((16, 32, 64, 128), (1, 1, 1, 1), v2), 7)
        with Record():
            for i in range(4):
                P.convnext_down_folded(sd, i)
                got = P.convnext_block_folded(sd, f"stages.{i}.0.")
        if v2:
            want = sd["stages.3.0.pwconv2.weight"].double() @ sd["stages.3.0.grn.beta"].double().flatten() + sd["stages.3.0.pwconv2.bias"].double()
            assert float((got[7] - want).abs().max()) < 1e-14
    assert seen and not {"matmul", "mm", "mv", "bmm", "addmm", "addmv", "linear", "einsum", "__matmul__", "__rmatmul__", "dot"} & set(seen), sorted(set(seen))


def test_argument_errors_come_before_device_work():
    from axial_vs_amd import _lib
    L = _lib.lib()
    p = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(6)]
    by = ctypes.byref
    outs = (ctypes.c_void_p * 5)(*[p[3]] * 5)

    def refused(rc, text):
        assert rc == -1 and text in L.axvs_last_error().decode(), (rc, L.axvs_last_error().decode())
    for bad, text in ((_cfg(dims=(16, 32, 64, 120)), "multiple of 16"), (_cfg(depths=(1, 1, 65, 1)), "blocks must be in 1..64"), (_cfg(N=0), "frames"),
                      (_cfg(h=(0, 2, 1, 1)), "pixels")):
        assert L.axvs_cnx_packed_bytes(by(bad)) == 0 or text in ("frames", "pixels")
        assert L.axvs_cnx_workspace_bytes(by(bad)) == 0
        refused(L.axvs_cnx_fwd(by(bad), p[0], p[1], outs, p[2], 1 << 40, None), text)
    refused(L.axvs_cnx_fwd(by(_cfg(h=(3, 2, 2, 1))), p[0], p[1], outs, p[2], 1 << 40, None), "gives 1 x 1")
    refused(L.axvs_cnx_fwd(by(_cfg()), None, p[1], outs, p[2], 1 << 40, None), "null pointer")
    refused(L.axvs_cnx_stem_fwd(by(_cfg(H=13)), p[0], p[1], p[3], p[2], 1 << 40, None), "stem's map")
    refused(L.axvs_cnx_down_fwd(by(_cfg()), p[0], 0, p[1], p[3], p[2], 1 << 40, None), "1..3")
    refused(L.axvs_cnx_down_fwd(by(_cfg(h=(3, 1, 1, 1))), p[0], 1, p[1], p[3], p[2], 1 << 40, None), "does not give")
    refused(L.axvs_cnx_dwln_fwd(by(_cfg()), p[0], 4, p[1], p[3], None), "block index")
    refused(L.axvs_cnx_dwln_fwd(by(_cfg()), p[0], 0, p[1], p[1], None), "out == x")
    refused(L.axvs_cnx_block_fwd(by(_cfg()), p[0], -1, p[1], p[3], p[2], 1 << 40, None), "block index")
    # a workspace one byte short: AXVS_ERR_WORKSPACE with both sizes in the text
    need = L.axvs_cnx_workspace_bytes(by(_cfg()))
    for rc in (L.axvs_cnx_fwd(by(_cfg()), p[0], p[1], outs, p[2], need - 1, None), L.axvs_cnx_stem_fwd(by(_cfg()), p[0], p[1], p[3], p[2], need - 1, None),
               L.axvs_cnx_down_fwd(by(_cfg()), p[0], 1, p[1], p[3], p[2], need - 1, None), L.axvs_cnx_block_fwd(by(_cfg()), p[0], 0, p[1], p[3], p[2], need - 1, None)):
        err = L.axvs_last_error().decode()
        assert rc == -2 and str(need - 1) in err and str(need) in err and "workspace too small" in err, (rc, err)


# ---- the cases can tell: each wrong form moves the float64 result by far more than the bound -----------------------------------------------
def test_cases_tell_a_wrong_halo():
    for spec in cc.DWLN_CASES:
        if spec[2] > 192:
            continue
        right, bad = cc.dwln_study(spec), cc.dwln_study(spec, "halo")
        assert cc.err(bad["out"], right["out"]) > 1000 * right["tol"], spec


def test_cases_tell_padded_pixels_as_zeros():
    for spec in cc.DOWN_CASES:
        right, bad = cc.down_study(spec), cc.down_study(spec, "pad_zero")
        d = cc.err(bad["out"], right["out"])
        if spec[0] % 2 or spec[1] % 2:
            assert d > 1000 * right["tol"], spec
        else:
            assert d == 0.0, spec             # no padded pixel in an even map
    st = cc.study(cc.BY_NAME["A_v1"])        # 17 x 25 -> 9 x 13 -> 5 x 7 -> 3 x 4: every downsample layer pads
    bad = cc.Restatement(st["params"], torch.float64, "pad_zero").forward(st["x"], cc.BY_NAME["A_v1"].depths)
    for k in ("res3", "res4", "res5"):
        assert cc.err(bad[k], st["want"][k]) > 1000 * st["tol"][k], k


def test_deep_cases_tell_a_dropped_k_step():
    """The cases at ConvNeXt-L's contraction depths (K = 3072, 6144) against a GEMM that stops one 32-wide k-step early: the float64 result
    moves by more than 100 x the case's bound -- in the whole blocks, in the deepest downsample layer, and in every step of the L
    networks' last two stages on the float64 chain."""
    for spec in cc.DEEP_BLOCK_CASES:
        right, bad = cc.block_study(spec[:4], C=spec[4]), cc.block_study(spec[:4], "k_short", C=spec[4])
        d = cc.err(bad["out"], right["out"])
        print(f"block {spec}: one k-step of {4 * spec[4] // 32} dropped moves float64 by {d:.3e} = {d / right['tol']:.0f} x the bound {right['tol']:.3e}")
        assert d > 100 * right["tol"], spec
    spec = cc.DOWN_CASES[-1]
    assert spec == (9, 13, 768)
    right, bad = cc.down_study(spec), cc.down_study(spec, "k_short")
    d = cc.err(bad["out"], right["out"])
    print(f"downsample {spec}: one k-step of {4 * spec[2] // 32} dropped moves float64 by {d:.3e} = {d / right['tol']:.0f} x the bound {right['tol']:.3e}")
    assert d > 100 * right["tol"], spec
    for case in cc.LARGE_NETS:
        st = cc.study(case)
        bad = cc.Restatement(st["params"], torch.float64, "k_short")
        seen = 0
        with torch.no_grad():
            for y in st["steps"]:
                stage = y["index"] if y["kind"] == "down" else y["index"][0]
                if stage < 2:
                    continue
                got = bad.down(y["x"].double(), stage) if y["kind"] == "down" else bad.block(y["x"].double(), f"stages.{stage}.{y['index'][1]}.")
                d = cc.err(got, y["out"])
                print(f"{case.name} {y['kind']} {y['index']}: one k-step dropped moves float64 by {d / y['tol']:.0f} x the bound {y['tol']:.3e}")
                assert d > 100 * y["tol"], (case.name, y["kind"], y["index"])
                seen += 1
        assert seen == 8          # two downsample layers (K = 1536, 3072), four blocks at K = 3072, two at K = 6144


def test_cases_tell_shared_grn_statistics():
    for spec in cc.BLOCK_CASES:
        if spec[3] != "v2" or spec[2] == 1:
            continue
        right, bad = cc.block_study(spec), cc.block_study(spec, "grn_shared")
        assert cc.err(bad["out"], right["out"]) > 1000 * right["tol"], spec
