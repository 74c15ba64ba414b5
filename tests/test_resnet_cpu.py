"""CPU: the restatement of the ResNet bottleneck backbone (tests/resnet_cases.py) against fixtures of the reference's own classes, the
module's state-dict names and shapes, its refusals, the new C-ABI symbols (axvs_rn_*) and their argument errors, which are reported
before any device work -- and that the cases can tell a wrong stride phase, a wrong dilation padding, a misplaced ReLU and (the blocks at
R-50's widths) a contraction one k-step short apart."""
import ctypes
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import resnet_cases as rc

from resnet_cases import GOLDEN, load_fixture, make_module, rn_cfg as _cfg

SYMBOLS = ["axvs_rn_packed_bytes", "axvs_rn_pack", "axvs_rn_workspace_bytes", "axvs_rn_fwd", "axvs_rn_stem_fwd", "axvs_rn_conv3_fwd", "axvs_rn_block_fwd"]


@pytest.fixture(scope="session", autouse=True)
def built():
    ge.build()


@pytest.mark.parametrize("fx", [c.name for c in rc.FIXTURES])
def test_restatement_equals_the_reference_bit_for_bit(fx):
    """The reference's own eval forward (fp32, CPU) against the float32 restatement on the same weights and input: the same ops in the
    same order, so the same bits -- on a CPU whose float32 kernels are the generator's (resnet_cases.cpu_probe); on every machine each
    output lies within 8 x the float32 restatement's own error against float64 of the reference's run."""
    case, m, z = load_fixture(fx)
    assert case == next(c for c in rc.FIXTURES if c.name == fx)
    assert m["keys"] == list(rc.param_shapes(case))
    st = rc.study(case)
    same_cpu = rc.cpu_probe() == m["probe"]
    for k in rc.OUTPUTS:
        ref = torch.from_numpy(z[k])
        e, own = rc.err(st["f32"][k], ref), st["tol"][k] / 8
        print(f"{fx} {k}: float32 restatement against the reference's fp32 run {e:.3e} (own error against float64 {own:.3e}); generator's CPU arithmetic: {same_cpu}")
        assert e <= 8 * own, k
        if same_cpu:
            assert torch.equal(st["f32"][k], ref), k
    assert os.path.getsize(os.path.join(GOLDEN, fx + ".npz")) < 512 * 1024


@pytest.mark.parametrize("fx", [c.name for c in rc.FIXTURES])
def test_state_dict_loads_strictly(fx):
    case, m, _ = load_fixture(fx)
    mod = make_module(case)
    assert list(mod.state_dict()) == m["keys"]
    ck = rc.net_params(case)
    mod.load_state_dict(ck, strict=True)
    assert torch.equal(mod.state_dict()["res4.1.conv2.weight"], ck["res4.1.conv2.weight"])
    assert torch.equal(mod.state_dict()["res3.0.shortcut.norm.running_var"], ck["res3.0.shortcut.norm.running_var"])


def test_r50_names_and_shapes():
    """R-50 on the meta device: the reference's key set, in its order, with its shapes (53 convolutions, each with its five BatchNorm
    entries); the BatchNorm's eps is the reference's 1e-3"""
    import axial_vs_amd as ax
    with torch.device("meta"):
        mod = ax.ResNetBackbone(depth=50)
    case = rc.Net("r50", 0, None, 1, 64, (64, 128, 256, 512), (256, 512, 1024, 2048), (3, 4, 6, 3), False, 1)
    want = rc.param_shapes(case)
    sd = mod.state_dict()
    assert len(sd) == 53 * 6 and list(sd) == list(want)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(s) for k, s in want.items()}
    assert tuple(sd["res5.0.shortcut.weight"].shape) == (2048, 1024, 1, 1) and "res5.1.shortcut.weight" not in sd
    assert mod.stem.conv1.norm.eps == 1e-3 and mod.res4[5].conv2.stride == (1, 1) and mod.res4[0].conv2.stride == (2, 2)
    with torch.device("meta"):
        msra = ax.ResNetBackbone(depth=101, stride_in_1x1=True, res5_dilation=2)
    assert len(msra.res4) == 23 and msra.res4[0].conv1.stride == (2, 2) and msra.res5[0].conv2.stride == (1, 1) and msra.res5[2].conv2.dilation == (2, 2)


def test_output_shape_and_size_divisibility():
    import axial_vs_amd as ax
    with torch.device("meta"):
        mod = ax.ResNetBackbone(depth=50, out_features=("stem", "res3", "res5"))
        dil = ax.ResNetBackbone(depth=50, res5_dilation=2)
    shp = mod.output_shape()
    assert list(shp) == ["stem", "res3", "res5"]
    assert [(s.channels, s.stride) for s in shp.values()] == [(64, 4), (512, 8), (2048, 32)]
    assert [(s.channels, s.stride) for s in dil.output_shape().values()] == [(256, 4), (512, 8), (1024, 16), (2048, 16)]
    assert mod.size_divisibility == 0
    assert type(shp["stem"]).__name__ == "ShapeSpec"
    assert rc.stage_sizes(rc.BY_NAME["A_a"], 769, 1345) == [(193, 337), (193, 337), (97, 169), (49, 85), (25, 43)]
    assert mod._conf.stage_sizes(769, 1345) == rc.stage_sizes(rc.BY_NAME["A_a"], 769, 1345)[:4]


@pytest.mark.parametrize("kw, text", [(dict(depth=18), "BasicBlock"), (dict(depth=34), "BasicBlock"), (dict(depth=77), "not one of"),
                                      (dict(num_groups=32, width_per_group=8), "ResNeXt"), (dict(deform_on_per_stage=(False, True, True, True)), "deformable"),
                                      (dict(res5_dilation=4), "res5_dilation 4"), (dict(norm="GN"), "norm 'GN'"), (dict(in_channels=4), "3-channel"),
                                      (dict(stem_out_channels=24), "multiple of 16 in 16..128"), (dict(stem_out_channels=256), "16..128"),
                                      (dict(width_per_group=48), "multiples of 32 in 32..512"), (dict(width_per_group=128), "32..512"),
                                      (dict(res2_out_channels=512), "16 in 16..2048"), (dict(num_blocks=(1, 1, 65, 1)), "1..64 blocks"),
                                      (dict(num_blocks=(1, 1, 1)), "four stages")])
def test_refusals_at_construction(kw, text):
    import axial_vs_amd as ax
    with torch.device("meta"), pytest.raises(NotImplementedError, match=text):
        ax.ResNetBackbone(**kw)
    with pytest.raises(ValueError, match="out_features"):
        with torch.device("meta"):
            ax.ResNetBackbone(out_features=("res6",))


def test_train_mode_and_cpu_tensors_raise():
    mod = make_module(rc.Net("t", 0, (8, 8), 1, 16, (32,) * 4, (32, 48, 64, 80), (1, 1, 1, 1), False, 1))
    assert mod.training
    with pytest.raises(NotImplementedError, match="eval"):
        mod(torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mod.eval()(torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError, match=r"\(N, 3, H, W\)"):
        mod(torch.zeros(1, 4, 8, 8))


def test_symbols_and_size_queries():
    from axial_vs_amd import _lib, _params as P
    L = _lib.lib()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(raw, s) and s in _lib.SIGNATURES, s
    cfg = _cfg()
    # every fp32 slot rounded up to 256 bytes; the 3x3 weight's slot holds 3 pieces x 2 bytes per value
    want = 5 * 3 * 512 * 2 + 256      # the stem: one n-tile of five 32-wide steps x 3 pieces x 512 16-bit values (K = 147 padded to 160), and its bias
    for cin, width, cout in ((16, 32, 32), (32, 32, 48), (48, 64, 64), (64, 64, 80)):
        for name, shape in P.resnet_block_shapes(cin, width, cout, True):
            want += ((6 if name == "w2" else 4) * int(np.prod(shape)) + 255) // 256 * 256
    assert L.axvs_rn_packed_bytes(ctypes.byref(cfg)) == want
    assert L.axvs_rn_workspace_bytes(ctypes.byref(cfg)) > 0
    assert [n for n, _ in P.resnet_block_shapes(16, 32, 32, True)] == list(_lib.RN_BLOCK_FIELDS)
    assert [n for n, _ in _lib.AxvsRnStemParams._fields_] == list(_lib.RN_STEM_FIELDS) == ["w", "b"]
    # R-50: 23.5 M convolution weights, the 3x3 ones (11.3 M) at 6 bytes, the others at 4
    r50 = _cfg(stem_channels=64, width=(64, 128, 256, 512), out_channels=(256, 512, 1024, 2048), blocks=(3, 4, 6, 3))
    assert 115e6 < L.axvs_rn_packed_bytes(ctypes.byref(r50)) < 120e6


def test_folded_parameters_have_the_stated_shapes_and_values():
    from axial_vs_amd import _params as P
    case = rc.Net("f", 5, None, 1, 16, (32, 32, 64, 64), (32, 48, 64, 80), (2, 1, 1, 1), False, 1)
    sd = rc.net_params(case)
    w, b = P.resnet_stem_folded(sd, rc.EPS)
    assert tuple(w.shape) == (147, 16) and tuple(b.shape) == (16,) and w.dtype == b.dtype == torch.float64
    scale = sd["stem.conv1.norm.weight"].double() / torch.sqrt(sd["stem.conv1.norm.running_var"].double() + rc.EPS)
    assert float(w[(2 * 7 + 3) * 7 + 5, 9]) == float(sd["stem.conv1.weight"][9, 2, 3, 5].double() * scale[9])
    assert torch.equal(b, sd["stem.conv1.norm.bias"].double() - sd["stem.conv1.norm.running_mean"].double() * scale)
    for p, cin, shortcut in (("res2.0.", 16, True), ("res2.1.", 32, False), ("res3.0.", 32, True)):
        got = P.resnet_block_folded(sd, p, rc.EPS)
        want = [s for _, s in P.resnet_block_shapes(cin, 32, 32 if p.startswith("res2") else 48, shortcut)]
        assert [None if t is None else tuple(t.shape) for t in got] == want
        assert all(t is None or t.dtype == torch.float64 for t in got)
    got = P.resnet_block_folded(sd, "res3.0.", rc.EPS)
    s2 = sd["res3.0.conv2.norm.weight"].double() / torch.sqrt(sd["res3.0.conv2.norm.running_var"].double() + rc.EPS)
    assert float(got[2][7, 2 * 3 + 1, 11]) == float(sd["res3.0.conv2.weight"][7, 11, 2, 1].double() * s2[7])      # (output channel, tap ky*3 + kx, input channel)
    # the fold is the eval BatchNorm: conv with the folded weight + bias equals batch_norm(conv) in float64
    x = torch.randn(1, 32, 5, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    r = rc.restatement(case, sd, torch.float64)
    want = r.bn(torch.nn.functional.conv2d(x, r.p["res3.0.conv2.weight"], None, padding=1), "res3.0.conv2.norm.")
    have = torch.nn.functional.conv2d(x, got[2].view(32, 3, 3, 32).permute(0, 3, 1, 2), got[3], padding=1)
    assert rc.err(have, want) < 1e-13


def test_argument_errors_come_before_device_work():
    from axial_vs_amd import _lib
    L = _lib.lib()
    p = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(6)]
    by = ctypes.byref
    outs = (ctypes.c_void_p * 5)(*[p[3]] * 5)
    big = 1 << 40

    def refused(rc_, text):
        assert rc_ == -1 and text in L.axvs_last_error().decode(), (rc_, L.axvs_last_error().decode())
    for bad, text in ((_cfg(blocks=(1, 0, 1, 1)), "blocks must be in 1..64"), (_cfg(blocks=(1, 65, 1, 1)), "blocks must be in 1..64"),
                      (_cfg(width=(32, 48, 64, 64)), "multiple of 32 in 32..512"), (_cfg(width=(32, 32, 64, 1024)), "multiple of 32 in 32..512"),
                      (_cfg(stem_channels=24), "multiple of 16 in 16..128"), (_cfg(stem_channels=144), "multiple of 16 in 16..128"),
                      (_cfg(out_channels=(32, 48, 64, 4096)), "multiple of 16 in 16..2048"), (_cfg(out_channels=(32, 40, 64, 80)), "multiple of 16 in 16..2048"),
                      (_cfg(in_channels=4), "3-channel images"), (_cfg(stride=(1, 3, 2, 2)), "stride 3 must be 1 or 2"),
                      (_cfg(dilation=(1, 1, 1, 3)), "dilation 3 must be 1 or 2"), (_cfg(out_channels=(32, 32, 64, 80)), "needs a projection shortcut"),
                      (_cfg(dilation=(1, 2, 1, 1)), "stride 2 together with dilation 2")):
        assert L.axvs_rn_packed_bytes(by(bad)) == 0 and L.axvs_rn_workspace_bytes(by(bad)) == 0
        refused(L.axvs_rn_fwd(by(bad), p[0], p[1], outs, None, p[2], big), text)
        refused(L.axvs_rn_pack(by(_lib.AxvsRnStemParams()), by(_lib.AxvsRnBlockParams()), by(bad), p[2], None), text)
    for bad, text in ((_cfg(N=0), "frames"), (_cfg(h=(0, 9, 5, 3)), "pixels")):
        assert L.axvs_rn_workspace_bytes(by(bad)) == 0
        refused(L.axvs_rn_fwd(by(bad), p[0], p[1], outs, None, p[2], big), text)
    refused(L.axvs_rn_fwd(by(_cfg(h=(9, 9, 4, 3))), p[0], p[1], outs, None, p[2], big), "stage 1 leaves 5 x 5")
    refused(L.axvs_rn_fwd(by(_cfg(H=37)), p[0], p[1], outs, None, p[2], big), "gives 10 x 9")
    refused(L.axvs_rn_fwd(by(_cfg()), None, p[1], outs, None, p[2], big), "null pointer")
    refused(L.axvs_rn_stem_fwd(by(_cfg(W=41)), p[0], p[1], p[3], None), "gives 9 x 11")
    refused(L.axvs_rn_conv3_fwd(by(_cfg()), p[0], 4, p[1], p[3], None), "block index")
    refused(L.axvs_rn_conv3_fwd(by(_cfg()), p[0], 0, p[1], p[1], None), "out == x")
    refused(L.axvs_rn_block_fwd(by(_cfg()), p[0], -1, p[1], p[3], None, p[2], big), "block index")
    # a workspace one byte short, and a negative size: AXVS_ERR_WORKSPACE with both sizes in the text
    need = L.axvs_rn_workspace_bytes(by(_cfg()))
    for have in (need - 1, -1):
        for rc_ in (L.axvs_rn_fwd(by(_cfg()), p[0], p[1], outs, None, p[2], have), L.axvs_rn_block_fwd(by(_cfg()), p[0], 0, p[1], p[3], None, p[2], have)):
            err = L.axvs_last_error().decode()
            assert rc_ == -2 and str(have) in err and str(need) in err and "workspace too small" in err, (rc_, err)


# ---- the cases can tell: each wrong form moves the float64 result by far more than the bound -----------------------------------------------
def test_cases_tell_a_wrong_stride_phase_and_dilation_padding():
    for spec in rc.CONV3_CASES:
        h, w, C, N, stride, d = spec
        if C > 160:
            continue
        right = rc.conv3_study(spec)
        if stride == 2 and max(h, w) > 1:
            assert rc.err(rc.conv3_study(spec, "stride_phase")["out"], right["out"]) > 1000 * right["tol"], spec
        if d == 2:
            assert rc.err(rc.conv3_study(spec, "dilation_pad")["out"], right["out"]) > 1000 * right["tol"], spec


def test_cases_tell_wrong_blocks():
    for spec in rc.BLOCK_CASES:
        h, w, N, kind = spec
        right = rc.block_study(spec)
        assert rc.err(rc.block_study(spec, "relu_before_add")["out"], right["out"]) > 1000 * right["tol"], spec
        if max(h, w) == 1:
            continue
        if kind in ("proj_s2", "s2_in_1x1"):
            assert rc.err(rc.block_study(spec, "shortcut_phase")["out"], right["out"]) > 1000 * right["tol"], spec
        if kind == "proj_s2":
            assert rc.err(rc.block_study(spec, "stride_phase")["out"], right["out"]) > 1000 * right["tol"], spec
        if kind == "dil2":
            assert rc.err(rc.block_study(spec, "dilation_pad")["out"], right["out"]) > 1000 * right["tol"], spec


def test_wide_cases_tell_a_dropped_k_step():
    """The blocks at R-50's own widths against a first 1x1 that stops one 32-wide k-step early (of 16, 32 and 64): the float64 result moves
    by more than 100 x the case's bound."""
    for spec in rc.WIDE_BLOCK_CASES:
        right, bad = rc.block_study(spec, net=rc.R50_WIDTHS), rc.block_study(spec, "k_short", net=rc.R50_WIDTHS)
        d = rc.err(bad["out"], right["out"])
        cin = right["x"].shape[-1]
        print(f"block {spec}: one k-step of {cin // 32} dropped moves float64 by {d:.3e} = {d / right['tol']:.0f} x the bound {right['tol']:.3e}")
        assert d > 100 * right["tol"], spec
    assert sorted({rc.block_study(s, net=rc.R50_WIDTHS)["x"].shape[-1] for s in rc.WIDE_BLOCK_CASES}) == [512, 1024, 2048]


def test_cases_tell_wrong_networks():
    case = rc.BY_NAME["A_a"]
    st = rc.study(case)
    for wrong, keys in (("stride_phase", ("res3", "res4", "res5")), ("shortcut_phase", ("res3", "res4", "res5")), ("relu_before_add", ("res2", "res5"))):
        bad = rc.restatement(case, st["params"], torch.float64, wrong).forward(st["x"], case.blocks)
        for k in keys:
            assert rc.err(bad[k], st["want"][k]) > 1000 * st["tol"][k], (wrong, k)
    case = rc.BY_NAME["A_b"]
    st = rc.study(case)
    bad = rc.restatement(case, st["params"], torch.float64, "dilation_pad").forward(st["x"], case.blocks)
    assert rc.err(bad["res5"], st["want"]["res5"]) > 1000 * st["tol"]["res5"]
    assert rc.err(bad["res4"], st["want"]["res4"]) == 0.0
