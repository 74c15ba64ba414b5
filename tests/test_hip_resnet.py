"""GPU: the ResNet bottleneck backbone (axial_vs_amd.ResNetBackbone, axvs_rn_*) against the float64 restatement of tests/resnet_cases.py.
Every bound is 8 x the float32 restatement's own max-norm error against float64, per compared tensor (9 x against fixtures of the
reference, whose fp32 run carries 1 x itself).  The restatements of a case run once (resnet_cases.study / *_study) and are shared.

Measured on an MI355X (profiles/resnet_parity.txt): every compared tensor sits inside its bound; the blocks at R-50's own widths
(WIDE_BLOCK_CASES, contractions of up to 2048 channels) at 1.6 .. 2.8 x (profiles/deep_contraction_parity.txt)."""
import ctypes

import pytest
import torch

import __graft_entry__ as ge
import resnet_cases as rc
from resnet_cases import load_fixture, make_module, rn_cfg as _cfg


@pytest.fixture(scope="session", autouse=True)
def built():
    ge.build()


def make(case, params, **kw):
    net = make_module(case, **kw)
    net.load_state_dict(params, strict=True)
    return net.cuda().eval()


ALL_OUT = dict(out_features=rc.OUTPUTS)
_DEVICE = {}


@pytest.fixture(scope="module", autouse=True)
def release_device_state():
    """this module's shared device state and the workspaces its largest cases grew are dropped when its tests are done, so that tests
    which measure peak device memory see what they saw before"""
    yield
    import gc
    _DEVICE.clear()
    rc._STUDY.clear()
    gc.collect()
    if torch.cuda.is_available():
        from axial_vs_amd import modules
        modules._workspaces.clear()
        torch.cuda.empty_cache()


def on_device(case):
    """(study, network with all five outputs, input) of a whole-network case, on the device once"""
    if case.name not in _DEVICE:
        st = rc.study(case)
        _DEVICE[case.name] = (st, make(case, st["params"], **ALL_OUT), st["x"].cuda())
    return _DEVICE[case.name]


def check(got, want, tol, what, factor=8):
    e = rc.err(got, want)
    print(f"{what}: max |device - float64| {e:.3e}, bound {tol:.3e} ({factor} x the float32 restatement's), ratio to that error {factor * e / tol:.2f}")
    assert tuple(got.shape) == tuple(want.shape), what
    assert e <= tol, what


@pytest.mark.gpu
@pytest.mark.parametrize("spec", rc.CONV3_CASES, ids=lambda s: "x".join(map(str, s)))
def test_conv3x3_teacher_forced(spec):
    """The implicit-GEMM 3x3 + folded BatchNorm + ReLU on float64 inputs: maps smaller than the halo, both parities at stride 2, one output
    pixel past whole tiles for every tile form, part tiles of output channels, every channel chunk, the real res5 maps."""
    st = rc.conv3_study(spec)
    check(make(st["case"], st["params"]).conv3x3(st["x"].cuda(), st["stage"], 0), st["out"], st["tol"], f"conv3x3 {spec}")


@pytest.mark.gpu
@pytest.mark.parametrize("size", rc.STEM_CASES, ids=lambda s: "x".join(map(str, s)))
def test_stem(size):
    """7x7 / stride 2 convolution + BatchNorm + ReLU + 3x3 / stride 2 max pool in one kernel: tiny images, all residues of H mod 4, one
    pooled pixel past the tile."""
    st = rc.stem_study(size)
    got = make(st["case"], st["params"]).stem_rows(st["x"].cuda())
    assert tuple(got.shape[1:3]) == rc.stage_sizes(st["case"], *size)[0]
    check(got, st["out"], st["tol"], f"stem {size}")


@pytest.mark.gpu
@pytest.mark.parametrize("spec", rc.BLOCK_CASES, ids=lambda s: "x".join(map(str, s)))
def test_block_teacher_forced(spec):
    """Whole blocks: identity shortcut, projection at stride 1 and 2 (odd and even maps), the stride in the first 1x1, dilation 2."""
    st = rc.block_study(spec)
    check(make(st["case"], st["params"]).block(st["x"].cuda(), st["stage"], st["index"]), st["out"], st["tol"], f"block {spec}")


@pytest.mark.gpu
@pytest.mark.parametrize("spec", rc.WIDE_BLOCK_CASES, ids=lambda s: "x".join(map(str, s)))
def test_wide_block_teacher_forced(spec):
    """Whole blocks at R-50's own widths, in both forms: res5's first block (the 1024 -> 2048 projection shortcut, the last 1x1 with the
    ReLU behind the residual), its second (the first 1x1 contracts over 2048 channels) and res4's first (test_resnet_cpu: one k-step
    less in the first 1x1 misses the bound by more than 100 x)."""
    st = rc.block_study(spec, net=rc.R50_WIDTHS)
    check(make(st["case"], st["params"]).block(st["x"].cuda(), st["stage"], st["index"]), st["out"], st["tol"], f"block {spec}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in rc.NETS])
def test_network_free_running(name):
    """The whole network against float64; the deep case (33 blocks) shows the error growth."""
    st, net, x = on_device(rc.BY_NAME[name])
    outs = net(x)
    assert list(outs) == list(rc.OUTPUTS)
    for k in rc.OUTPUTS:
        check(outs[k], st["want"][k], st["tol"][k], f"{name} {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A_a", "A_b"])
def test_steps_teacher_forced(name):
    """The stem, every 3x3 and every block of the network on the float64 chain's inputs."""
    st, net, _ = on_device(rc.BY_NAME[name])
    for y in st["steps"]:
        x = y["x"].cuda()
        if y["kind"] == "stem":
            got = net.stem_rows(x)
        elif y["kind"] == "conv3":
            got = net.conv3x3(rc.rows(x), *y["index"])
        else:
            got = net.block(rc.rows(x), *y["index"])
        check(got, rc.rows(y["out"]), y["tol"], f"{name} {y['kind']} {y['index']}")


@pytest.mark.gpu
@pytest.mark.parametrize("fx", [c.name for c in rc.FIXTURES])
def test_against_reference_fixture(fx):
    """The device against the reference's own fp32 run: 9 x the float32 restatement's error (the reference's run carries 1 x itself)."""
    case, m, z = load_fixture(fx)
    st, net, x = on_device(case)
    outs = net(x)
    for k in rc.OUTPUTS:
        check(outs[k], torch.from_numpy(z[k]), 9 * st["tol"][k] / 8, f"{fx} {k}", factor=9)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["C_a", "C_b"])
def test_bit_equality(name):
    """Run to run; stacked frames against single frames; a channels_last image against a contiguous one; out_features subsets against
    the full run; the functional form against the module."""
    case = rc.BY_NAME[name]
    st, net, x = on_device(case)
    a, b = net(x), net(x)
    for k in rc.OUTPUTS:
        assert torch.equal(a[k], b[k]), k
    for n in range(case.N):
        one = net(x[n:n + 1])
        for k in rc.OUTPUTS:
            assert torch.equal(one[k][0], a[k][n]), (k, n)
    cl = net(x.contiguous(memory_format=torch.channels_last))
    for k in rc.OUTPUTS:
        assert torch.equal(cl[k], a[k]), k
    for sub in (("res2", "res3", "res4", "res5"), ("res5",), ("res3", "stem")):
        part = make(case, st["params"], out_features=sub)(x)
        assert list(part) == list(sub)
        for k in part:
            assert torch.equal(part[k], a[k]), (sub, k)
    import axial_vs_amd as ax
    fn = ax.resnet_forward({k: v.cuda() for k, v in st["params"].items()}, x, rc.OUTPUTS, stride_in_1x1=case.stride_in_1x1, res5_dilation=case.res5_dilation)
    assert list(fn) == list(rc.OUTPUTS)
    for k in rc.OUTPUTS:
        assert torch.equal(fn[k], a[k]), k


@pytest.mark.gpu
def test_repack_on_parameter_and_statistic_change():
    case = rc.BY_NAME["B_a"]
    st = rc.study(case)
    net = make(case, st["params"], **ALL_OUT)
    x = st["x"].cuda()
    a = net(x)
    with torch.no_grad():
        net.res5[0].conv2.weight.mul_(2.0)
    b = net(x)
    assert torch.equal(a["res4"], b["res4"]) and not torch.equal(a["res5"], b["res5"])
    with torch.no_grad():
        net.res4[1].conv3.norm.running_mean.add_(0.5)          # a buffer, not a parameter: folded all the same
    c = net(x)
    assert torch.equal(b["res3"], c["res3"]) and not torch.equal(b["res4"], c["res4"])


@pytest.mark.gpu
def test_chain_to_the_pixel_decoder():
    """The output dict feeds KMaXPixelDecoder.forward_features as it is (R-50's channel counts at a quarter of its bottleneck widths, the
    pixel decoder's case A): the decoder's outputs equal those of the same call on copies of the tensors."""
    import axial_vs_amd as ax
    import kmax_pixel_decoder_cases as pc
    pcase = pc.BY_NAME["A"]
    case = rc.Net("chain", 2890, pcase.spatial, 2, 16, (32, 32, 64, 128), tuple(pcase.in_channels), (1, 1, 1, 1), False, 1)
    net = make(case, rc.net_params(case))
    x = torch.randn(2, 3, *pcase.spatial, generator=torch.Generator().manual_seed(2891)).cuda()
    feats = net(x)
    assert list(feats) == ["res2", "res3", "res4", "res5"]
    assert [tuple(feats[f"res{5 - i}"].shape[-2:]) for i in range(4)] == pc.query_shapes(pcase.spatial)
    dec = ax.KMaXPixelDecoder(net.output_shape(), pcase.dec_layers, pcase.dec_channels, pcase.layer_types, pcase.spatial)
    dec.load_state_dict(pc.make_params(pcase), strict=True)
    dec = dec.cuda().eval()
    pan, sem, ms = dec.forward_features(feats)
    pan2, _, ms2 = dec.forward_features({k: v.clone() for k, v in feats.items()})
    assert torch.isfinite(pan).all() and sem[0] is feats["res5"]
    for a, b in zip([pan] + list(ms), [pan2] + list(ms2)):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_abi_refusals_with_device_pointers():
    """The C entry points with real device buffers: a refused call returns AXVS_ERR_ARG / AXVS_ERR_WORKSPACE with its message and leaves the
    output untouched; the same call with a valid configuration runs."""
    from axial_vs_amd import _lib
    L = _lib.lib()
    by = ctypes.byref
    case = rc.Net("abi", 2895, (33, 33), 1, 16, (32, 32, 64, 64), (32, 48, 64, 80), (1, 1, 1, 1), False, 1)
    net = make(case, rc.net_params(case), **ALL_OUT)
    x = torch.randn(1, 3, 33, 33, generator=torch.Generator().manual_seed(2896)).cuda()
    want = net(x)
    packed = net._packed()
    good = _cfg()
    need = L.axvs_rn_workspace_bytes(by(good))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    outs = {k: torch.full_like(v, 7.0) for k, v in want.items()}
    op = (ctypes.c_void_p * 5)(*[outs[k].data_ptr() for k in rc.OUTPUTS])
    st = torch.cuda.current_stream().cuda_stream
    for bad, code, text in ((_cfg(width=(32, 48, 64, 64)), -1, "multiple of 32"), (_cfg(blocks=(1, 65, 1, 1)), -1, "1..64"), (_cfg(H=37), -1, "gives 10 x 9"),
                            (_cfg(stem_channels=8), -1, "16..128"), (_cfg(in_channels=1), -1, "3-channel")):
        rc_ = L.axvs_rn_fwd(by(bad), packed.data_ptr(), x.data_ptr(), op, st, ws.data_ptr(), need)
        assert rc_ == code and text in L.axvs_last_error().decode(), (rc_, L.axvs_last_error().decode())
    assert L.axvs_rn_fwd(by(good), packed.data_ptr(), x.data_ptr(), op, st, ws.data_ptr(), need - 1) == -2
    assert L.axvs_rn_block_fwd(by(good), packed.data_ptr(), 4, x.data_ptr(), outs["res2"].data_ptr(), st, ws.data_ptr(), need) == -1
    torch.cuda.synchronize()
    assert all(bool((v == 7.0).all()) for v in outs.values())
    assert L.axvs_rn_fwd(by(good), packed.data_ptr(), x.data_ptr(), op, st, ws.data_ptr(), need) == 0
    torch.cuda.synchronize()
    for k in rc.OUTPUTS:
        assert torch.equal(outs[k], want[k]), k


@pytest.mark.gpu
def test_r50_runs_a_small_frame():
    """R-50 itself (every stage's real widths, the 64-channel tile form of the 3x3 included) on one small frame: shapes, finite, and
    non-negative behind the last ReLU"""
    import axial_vs_amd as ax
    torch.manual_seed(2897)
    net = ax.ResNetBackbone(depth=50, out_features=rc.OUTPUTS)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_var.uniform_(0.5, 1.5), m.running_mean.uniform_(-0.3, 0.3), m.bias.uniform_(-0.2, 0.2)
    net = net.cuda().eval()
    outs = net(torch.randn(1, 3, 64, 96, device="cuda"))
    assert [tuple(v.shape) for v in outs.values()] == [(1, 64, 16, 24), (1, 256, 16, 24), (1, 512, 8, 12), (1, 1024, 4, 6), (1, 2048, 2, 3)]
    assert all(bool(torch.isfinite(v).all()) and float(v.min()) >= 0.0 for v in outs.values())
