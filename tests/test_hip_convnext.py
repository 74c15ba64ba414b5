"""GPU: the ConvNeXt / ConvNeXtV2 backbone (axial_vs_amd.ConvNeXtBackbone / ConvNeXtV2Backbone, axvs_cnx_*) against the float64
restatement of tests/convnext_cases.py.  Every bound is 8 x the float32 restatement's own max-norm error against float64, per compared
tensor (9 x against fixtures of the reference, whose fp32 run carries 1 x itself).  The restatements of a case run once
(convnext_cases.study / *_study) and are shared.

Measured on an MI355X (profiles/convnext_parity.txt): every compared tensor sits inside its bound.  The cases at ConvNeXt-L's widths
(DEEP_BLOCK_CASES, the 9 x 13 x 768 downsample layer, L_v1 / L_v2) hold the GEMM's contractions over 3072 and 6144 inputs to the same
bound (profiles/deep_contraction_parity.txt: the downsample layer sat at 10.1 x before the GEMM's step sums, every one at 1.2 .. 6.0 x
since)."""
import pytest
import torch

import __graft_entry__ as ge
import convnext_cases as cc
from test_convnext_cpu import load_fixture


@pytest.fixture(scope="session", autouse=True)
def built():
    ge.build()


def make(dims, depths, v2, params, gamma=True, **kw):
    import axial_vs_amd as ax
    if v2:
        net = ax.ConvNeXtV2Backbone(depths=depths, dims=dims, **kw)
    else:
        net = ax.ConvNeXtBackbone(depths=depths, dims=dims, layer_scale_init_value=1e-6 if gamma else 0.0, **kw)
    net.load_state_dict(params, strict=True)
    return net.cuda().eval()


ALL_OUT = dict(out_features=cc.OUTPUTS)
_DEVICE = {}


@pytest.fixture(scope="module", autouse=True)
def release_device_state():
    """this module's shared device state (the L cases' networks among it: 0.25 GB of parameters each, and as much again packed) and the
    scratch buffer its largest case grew (the hidden rows of the 25 x 43 x 1536 map) are dropped when its tests are done, so that tests
    which measure peak device memory see what they saw before"""
    yield
    import gc
    _DEVICE.clear()
    cc._STUDY.clear()
    gc.collect()
    if torch.cuda.is_available():
        from axial_vs_amd import modules
        modules._workspaces.clear()
        torch.cuda.empty_cache()


def on_device(case):
    """(study, network with all five outputs, input) of a whole-network case, on the device once"""
    if case.name not in _DEVICE:
        st = cc.study(case)
        _DEVICE[case.name] = (st, make(case.dims, case.depths, case.v2, st["params"], case.gamma, **ALL_OUT), st["x"].cuda())
    return _DEVICE[case.name]


def check(got, want, tol, what, factor=8):
    e = cc.err(got, want)
    print(f"{what}: max |device - float64| {e:.3e}, bound {tol:.3e} ({factor} x the float32 restatement's), ratio to that error {factor * e / tol:.2f}")
    assert tuple(got.shape) == tuple(want.shape), what
    assert e <= tol, what


def stage_net(st, v2=False, gamma=True):
    return make(st["dims"], (1, 1, 1, 1), v2, st["params"], gamma)


@pytest.mark.gpu
@pytest.mark.parametrize("spec", cc.DWLN_CASES, ids=lambda s: "x".join(map(str, s)))
def test_dwconv_norm_teacher_forced(spec):
    """The fused depthwise 7x7 + LayerNorm on float64 inputs: maps smaller than the halo, the tile size + 1, every channel chunk."""
    st = cc.dwln_study(spec)
    check(stage_net(st).dwconv_norm(st["x"].cuda(), 0, 0), st["out"], st["tol"], f"dwconv + norm {spec}")


@pytest.mark.gpu
@pytest.mark.parametrize("size", cc.STEM_CASES, ids=lambda s: "x".join(map(str, s)))
def test_stem(size):
    """The stem behind F.pad(x, (1, 2, 1, 2)): all four residues of (H + 3) mod 4."""
    st = cc.stem_study(size)
    got = stage_net(st).stem(st["x"].cuda())
    assert tuple(got.shape[1:3]) == cc.map_sizes(*size)[0]
    check(got, st["out"], st["tol"], f"stem {size}")


@pytest.mark.gpu
@pytest.mark.parametrize("spec", cc.DOWN_CASES, ids=lambda s: "x".join(map(str, s)))
def test_downsample(spec):
    """A downsample layer behind F.pad(x, (0, 1, 0, 1)) in front of its LayerNorm.  The whole output is compared: the last row and column
    of an odd map's output read the padded positions (test_convnext_cpu: zeros there instead of the LayerNorm's bias miss the bound by
    more than 1000 x)."""
    st = cc.down_study(spec)
    net = stage_net(st)
    check(net.downsample(st["x"].cuda(), 1), st["out"], st["tol"], f"downsample {spec}")


@pytest.mark.gpu
@pytest.mark.parametrize("spec", cc.BLOCK_CASES, ids=lambda s: "x".join(map(str, s)))
def test_block_teacher_forced(spec):
    """Whole blocks (v1, v2, v1 without gamma); for v2 the frames differ in scale, so shared or swapped GRN statistics fail."""
    st = cc.block_study(spec)
    check(stage_net(st, st["v2"], st["gamma"]).block(st["x"].cuda(), 0, 0), st["out"], st["tol"], f"block {spec}")


@pytest.mark.gpu
@pytest.mark.parametrize("spec", cc.DEEP_BLOCK_CASES, ids=lambda s: "x".join(map(str, s)))
def test_deep_block_teacher_forced(spec):
    """Whole blocks at the widths of ConvNeXt-L's last two stages: `pwconv2` contracts over 3072 and 6144 inputs, 96 and 192 k-steps of
    the three-piece GEMM in one accumulator (test_convnext_cpu: one k-step less misses the bound by more than 100 x)."""
    st = cc.block_study(spec[:4], C=spec[4])
    check(stage_net(st, st["v2"], st["gamma"]).block(st["x"].cuda(), 0, 0), st["out"], st["tol"], f"block {spec}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in cc.NETS + cc.LARGE_NETS])
def test_network_free_running(name):
    """The whole network against float64; the deep cases (36 blocks) show the error growth, the L cases the growth over four blocks that
    contract over 3072 and two over 6144."""
    st, net, x = on_device(cc.BY_NAME[name])
    outs = net(x)
    assert list(outs) == list(cc.OUTPUTS)
    for k in cc.OUTPUTS:
        check(outs[k], st["want"][k], st["tol"][k], f"{name} {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A_v1", "A_v2", "L_v1", "L_v2"])
def test_steps_teacher_forced(name):
    """Every downsample layer and every block of the network on the float64 chain's inputs."""
    st, net, _ = on_device(cc.BY_NAME[name])
    for y in st["steps"]:
        x = y["x"].cuda()
        if y["kind"] == "down":
            got = net.stem(x) if y["index"] == 0 else net.downsample(cc.rows(x), y["index"])
        else:
            got = net.block(cc.rows(x), *y["index"])
        check(got, cc.rows(y["out"]), y["tol"], f"{name} {y['kind']} {y['index']}")


@pytest.mark.gpu
@pytest.mark.parametrize("fx", [c.name for c in cc.FIXTURES])
def test_against_reference_fixture(fx):
    """The device against the reference's own fp32 run: 9 x the float32 restatement's error (the reference's run carries 1 x itself)."""
    case, m, z = load_fixture(fx)
    st, net, x = on_device(case)
    outs = net(x)
    for k in cc.OUTPUTS:
        check(outs[k], torch.from_numpy(z[k]), 9 * st["tol"][k] / 8, f"{fx} {k}", factor=9)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["C_v1", "C_v2"])
def test_bit_equality(name):
    """Run to run; stacked frames against single frames; a channels_last image against a contiguous one; out_features subsets and the stem
    against the full run."""
    case = cc.BY_NAME[name]
    st, net, x = on_device(case)
    a, b = net(x), net(x)
    for k in cc.OUTPUTS:
        assert torch.equal(a[k], b[k]), k
    for n in range(case.N):
        one = net(x[n:n + 1])
        for k in cc.OUTPUTS:
            assert torch.equal(one[k][0], a[k][n]), (k, n)
    cl = net(x.contiguous(memory_format=torch.channels_last))
    for k in cc.OUTPUTS:
        assert torch.equal(cl[k], a[k]), k
    for sub in (("res2", "res3", "res4", "res5"), ("res5",), ("stem", "res3")):
        part = make(case.dims, case.depths, case.v2, st["params"], case.gamma, out_features=sub)(x)
        assert list(part) == [k for k in cc.OUTPUTS if k in sub]
        for k in part:
            assert torch.equal(part[k], a[k]), (sub, k)
    idx = make(case.dims, case.depths, case.v2, st["params"], case.gamma, out_indices=(1, 3), **ALL_OUT)(x)
    assert list(idx) == ["stem", "res3", "res5"]
    import axial_vs_amd as ax
    fn = ax.convnext_forward({k: v.cuda() for k, v in st["params"].items()}, x, cc.OUTPUTS)
    for k in cc.OUTPUTS:
        assert torch.equal(fn[k], a[k]), k


@pytest.mark.gpu
def test_repack_on_parameter_change():
    case = cc.BY_NAME["B_v2"]
    st = cc.study(case)
    net = make(case.dims, case.depths, case.v2, st["params"], **ALL_OUT)
    x = st["x"].cuda()
    a = net(x)
    with torch.no_grad():
        net.stages[3][0].grn.gamma.mul_(2.0)
    b = net(x)
    assert torch.equal(a["res4"], b["res4"]) and not torch.equal(a["res5"], b["res5"])


@pytest.mark.gpu
def test_chain_to_the_pixel_decoder():
    """The output dict feeds KMaXPixelDecoder.forward_features as it is (dims of ConvNeXt-L, case C's channel counts and size): the decoder's
    outputs equal those of the same call on copies of the tensors."""
    import axial_vs_amd as ax
    import kmax_pixel_decoder_cases as pc
    pcase = pc.BY_NAME["C"]
    dims = pcase.in_channels
    params = cc.draw(cc.param_shapes(dims, (1, 1, 1, 1), True), 2790)
    net = make(dims, (1, 1, 1, 1), True, params)
    x = torch.randn(2, 3, *pcase.spatial, generator=torch.Generator().manual_seed(2791)).cuda()
    feats = net(x)
    assert [tuple(feats[f"res{5 - i}"].shape[-2:]) for i in range(4)] == pc.query_shapes(pcase.spatial)
    dec = ax.KMaXPixelDecoder(net.output_shape(), pcase.dec_layers, pcase.dec_channels, pcase.layer_types, pcase.spatial)
    dec.load_state_dict(pc.make_params(pcase), strict=True)
    dec = dec.cuda().eval()
    pan, sem, ms = dec.forward_features(feats)
    pan2, _, ms2 = dec.forward_features({k: v.clone() for k, v in feats.items()})
    assert torch.isfinite(pan).all() and sem[0] is feats["res5"]
    for a, b in zip([pan] + list(ms), [pan2] + list(ms2)):
        assert torch.equal(a, b)
