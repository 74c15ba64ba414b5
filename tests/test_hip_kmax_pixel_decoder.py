"""GPU: Video-kMaX's pixel decoder (axial_vs_amd.KMaXPixelDecoder, axvs_kmax_pix_*) and the head chain (MaXTronDeepLabHead) against the
float64 restatement of tests/kmax_pixel_decoder_cases.py.  Every bound is 8 x the float32 restatement's own max-norm error against float64,
per compared tensor (9 x against fixtures of the reference, whose fp32 run carries 1 x itself).  The restatements of a case run once
(kmax_pixel_decoder_cases.study / stage_study) and are shared."""
import types

import pytest
import torch

import __graft_entry__ as ge
import kmax_pixel_decoder_cases as pc
from test_kmax_pixel_decoder_cpu import check_against_fixture, load_fixture


@pytest.fixture(scope="session", autouse=True)
def built():
    ge.build()


def make_decoder(case, params):
    import axial_vs_amd as ax
    dec = ax.KMaXPixelDecoder(pc.input_shape(case), case.dec_layers, case.dec_channels, case.layer_types, case.spatial or (64, 64))
    dec.load_state_dict(params, strict=True)
    return dec.cuda().eval()


_DEVICE = {}


@pytest.fixture(scope="module", autouse=True)
def release_device_state():
    """a decoder is ~170 MB of parameters and packed weights: this module's shared device state is dropped when its tests are done, so
    that tests which measure peak device memory see what they saw before"""
    yield
    _DEVICE.clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def on_device(case):
    """(study, decoder, features) of a whole-decoder case, on the device once"""
    if case.name not in _DEVICE:
        st = pc.study(case)
        _DEVICE[case.name] = (st, make_decoder(case, st["params"]), {k: v.cuda() for k, v in st["feats"].items()})
    return _DEVICE[case.name]


def run(dec, feats):
    pan, sem, ms = dec.forward_features(dict(feats))
    return dict(zip(pc.OUTPUTS, list(ms) + [pan])), sem


def check(got, want, tol, what):
    e = pc.err(got, want)
    print(f"{what}: max |device - float64| {e:.3e}, bound {tol:.3e} (8 x the float32 restatement's), ratio to that error {8 * e / tol:.2f}")
    assert tuple(got.shape) == tuple(want.shape), what
    assert e <= tol, what


ALL = [c.name for c in pc.CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("spec", pc.AXIAL_STAGE_CASES, ids=lambda s: "x".join(map(str, s)))
def test_axial_attn_teacher_forced(spec):
    """One axis pass of each axis on the float64 chain's qkv rows."""
    st = pc.stage_study("axial", spec)
    dec = make_decoder(st["case"], st["params"])
    for axis, ax in enumerate("hw"):
        got = dec.axial_attn(st["rec"]["qkv_" + ax].float().contiguous().cuda(), 0, 0, axis)
        check(got, st["rec"]["out_" + ax], st["tol_" + ax], f"axis {ax} {spec}")


@pytest.mark.gpu
@pytest.mark.parametrize("spec", pc.AXIAL_STAGE_CASES, ids=lambda s: "x".join(map(str, s)))
def test_axial_block(spec):
    st = pc.stage_study("axial", spec)
    dec = make_decoder(st["case"], st["params"])
    check(dec.block(st["x"].cuda(), 0, 0), st["out"], st["tol"], f"axial block {spec}")


@pytest.mark.gpu
@pytest.mark.parametrize("spec", pc.BOTTLENECK_STAGE_CASES, ids=lambda s: "x".join(map(str, s)))
def test_bottleneck_block(spec):
    st = pc.stage_study("bottleneck", spec)
    dec = make_decoder(st["case"], st["params"])
    check(dec.block(st["x"].cuda(), 3, 0), st["out"], st["tol"], f"bottleneck block {spec}")


@pytest.mark.gpu
@pytest.mark.parametrize("spec", pc.FUSE_STAGE_CASES, ids=lambda s: f"{s[0][0]}x{s[0][1]}_{s[2]}_{s[3]}_{s[4]}")
def test_fuse(spec):
    """One ResizedFuse with the LayerNorm of its high-resolution input; the last two cases lack the high / the low convolution."""
    st = pc.stage_study("fuse", spec)
    dec = make_decoder(st["case"], st["params"])
    check(dec.fuse(st["low"].cuda(), st["high"].cuda(), 0), st["out"], st["tol"], f"fuse {spec}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_steps_teacher_forced(name):
    """Every block and every fuse of the decoder on the float64 chain's inputs."""
    st, dec, feats = on_device(pc.BY_NAME[name])
    for y in st["steps"]:
        if y["kind"] == "fuse":
            got = dec.fuse(y["low"].float().cuda(), y["high"].cuda(), y["index"])
            check(got, y["out"], y["tol"], f"{name} fuse {y['index']}")
        else:
            got = dec.block(y["x"].float().cuda(), y["stage"], y["index"])
            check(got, y["out"], y["tol"], f"{name} stage {y['stage']} block {y['index']}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_decoder_free_running(name):
    st, dec, feats = on_device(pc.BY_NAME[name])
    out, sem = run(dec, feats)
    for k in pc.OUTPUTS:
        check(out[k], st["out"][k], st["tol"][k], f"{name} {k}")
    assert sem[0] is feats["res5"] and sem[1] is feats["res3"] and sem[2] is feats["res2"]        # the caller's own tensors


@pytest.mark.gpu
@pytest.mark.parametrize("fx", [c.name for c in pc.FIXTURES])
def test_fixtures_of_the_reference(fx):
    case, m, z = load_fixture(fx)
    st, dec, feats = on_device(case)
    out, _ = run(dec, feats)
    check_against_fixture(z, out, st, 9, fx)


@pytest.mark.gpu
def test_functional_form_equals_the_module():
    import axial_vs_amd as ax
    case = pc.BY_NAME["A"]
    st, dec, feats = on_device(case)
    out, _ = run(dec, feats)
    params = {k: v.cuda() for k, v in st["params"].items()}
    pan, sem, ms = ax.kmax_pixel_decoder_forward(params, feats, case.dec_layers, case.dec_channels, case.layer_types, case.spatial)
    for k, t in zip(pc.OUTPUTS, list(ms) + [pan]):
        assert torch.equal(t, out[k]), k
    assert sem[0] is feats["res5"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "C"])
def test_runs_and_stacked_frames_are_bit_equal(name):
    """Two runs give equal bits; a stacked batch gives the bits of its frames run singly."""
    st, dec, feats = on_device(pc.BY_NAME[name])
    a, _ = run(dec, feats)
    b, _ = run(dec, feats)
    for k in pc.OUTPUTS:
        assert torch.equal(a[k], b[k]), k
    for n in range(st["case"].N):
        one, _ = run(dec, {k: v[n:n + 1].contiguous() for k, v in feats.items()})
        for k in pc.OUTPUTS:
            assert torch.equal(one[k][0], a[k][n]), (k, n)


@pytest.mark.gpu
def test_non_default_stream():
    st, dec, feats = on_device(pc.BY_NAME["B"])
    a, _ = run(dec, feats)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b, _ = run(dec, feats)
    s.synchronize()
    for k in pc.OUTPUTS:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
def test_parameter_change_is_picked_up():
    """An in-place change bumps the parameter's version: the next forward packs again; `invalidate_pack` forces it for a change made
    behind autograd's back."""
    import axial_vs_amd as ax
    case = pc.BY_NAME["B"]
    st = pc.study(case)
    dec = make_decoder(case, st["params"])
    feats = {k: v.cuda() for k, v in st["feats"].items()}
    a, _ = run(dec, feats)
    w = dec._stages[3]._blocks[0]._conv3_bn.norm.weight
    w.data.mul_(2.0)                        # .data: no version bump
    ax.invalidate_pack(dec)
    b, _ = run(dec, feats)
    assert torch.equal(a["stage2"], b["stage2"]) and not torch.equal(a["panoptic"], b["panoptic"])
    params = dict(st["params"])
    params["_stages.3._blocks.0._conv3_bn.norm.weight"] = params["_stages.3._blocks.0._conv3_bn.norm.weight"] * 2.0
    want = pc.Restatement(params, torch.float64).run(st["feats"], case.dec_layers)[1][-1]
    want32 = pc.Restatement(params, torch.float32).run(st["feats"], case.dec_layers)[1][-1]
    check(b["panoptic"], want, 8 * pc.err(want32, want), "after the change")
    with torch.no_grad():
        dec._stages[0]._blocks[0]._attention._height_axis._batch_norm_similarity.running_var.add_(0.5)      # a buffer, in place
    c, _ = run(dec, feats)
    assert not torch.equal(b["stage0"], c["stage0"])


def _predictor(in_channels, frames):
    import axial_vs_amd as ax
    import kmax_decoder_cases as kc
    case = kc.Case("head", 2650, 16, 4, frames, None, None, tuple(in_channels), (1, 1, 1), 1, 0.1)
    dec = ax.KMaXTransformerDecoder(case.dec_layers, case.in_channels, case.K, case.L, case.T, False)
    dec.load_state_dict(kc.make_params(case), strict=True)
    return dec.cuda().eval()


@pytest.mark.gpu
def test_head_without_within_clip_module():
    """`layers` chains the pixel decoder and the query decoder: bit-equal to calling the two by hand."""
    import axial_vs_amd as ax
    st, dec, feats = on_device(pc.BY_NAME["A"])
    pred = _predictor((2048, 1024, 512), 2)
    head = ax.MaXTronDeepLabHead(None, dec, pred).eval()
    got = head(dict(feats))
    pan, sem, ms = dec.forward_features(dict(feats))
    want = pred(ms, pan, sem)
    assert set(got) == set(want)
    for k in ("pred_logits", "pred_masks", "pred_mask_embeddings", "pixel_feature", "cluster_centers"):
        assert torch.equal(got[k], want[k]), k
    assert tuple(got["pred_masks"].shape) == (1, 16, 2, 17, 25) and bool(torch.isfinite(got["pred_masks"]).all())
    assert head.layers(dict(feats))["pred_logits"].equal(want["pred_logits"])


@pytest.mark.gpu
def test_head_with_within_clip_module():
    """The three steps under the reference's names, the within-clip module at the size tests/test_hip_packs.py builds it."""
    import axial_vs_amd as ax
    S = lambda c, s: types.SimpleNamespace(channels=c, stride=s)
    torch.manual_seed(2660)
    wc = ax.WithinClipTrackingModule(
        {"res3": S(32, 8), "res4": S(64, 16), "res5": S(64, 32)}, transformer_dropout=0.0, transformer_attn_drop=0.0, transformer_nheads=8,
        transformer_dim_feedforward=128, transformer_num_stages=1, transformer_spatial_layers=1, transformer_temporal_layers=1,
        transformer_temporal_attn_type="axial-trajectory", transformer_conv_dims=64, transformer_spatial_in_features=["res3", "res4", "res5"],
        transformer_temporal_in_features=["res4", "res5"], num_clip_frames=2, cross_clip_training=False).cuda().eval()
    case = pc.Case("head_wc", 2661, (64, 96), 2, (16, 32, 64, 64), (1, 1, 1, 1), (128, 128, 32, 64), ("axial", "axial", "bottleneck", "bottleneck"))
    dec = make_decoder(case, pc.make_params(case))
    pred = _predictor((512, 512, 128), 2)
    head = ax.MaXTronDeepLabHead(wc, dec, pred).eval()
    feats = {k: v.cuda() for k, v in pc.make_inputs(case).items()}
    got = head(dict(feats))
    f2, _, _ = wc.forward_features(dict(feats))
    assert not torch.equal(f2["res5"], feats["res5"]) and f2["res2"] is feats["res2"]
    pan, sem, ms = dec.forward_features(f2)
    want = pred(ms, pan, sem)
    for k in ("pred_logits", "pred_masks", "pred_mask_embeddings", "pixel_feature", "cluster_centers"):
        assert torch.equal(got[k], want[k]) and bool(torch.isfinite(got[k]).all()), k
    # the pixel decoder inside the chain against the float64 restatement on the within-clip module's features
    st_feats = {k: v.detach().cpu() for k, v in f2.items()}
    params = pc.make_params(case)
    out64 = pc.Restatement(params, torch.float64).run(st_feats, case.dec_layers)[1]
    out32 = pc.Restatement(params, torch.float32).run(st_feats, case.dec_layers)[1]
    check(pan, out64[-1], 8 * pc.err(out32[-1], out64[-1]), "panoptic features in the chain")
