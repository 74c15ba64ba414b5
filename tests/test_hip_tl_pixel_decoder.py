"""GPU: Tube-Link's pixel decoder (axial_vs_amd.TubeLinkPixelDecoder) and its new library pieces -- the FPN level
(axvs_fpn_level_fwd: lateral 1x1 conv + GN + bilinear merge, 3x3 conv + GN + ReLU, mask_feature) and the stand-alone FFN tail pack
(axvs_ffn_pack / axvs_ffn_packed_fwd) -- against float64 restatements of TL/mmdet/models/plugins/msdeformattn_pixel_decoder.py:311-325."""
import ctypes as C
import copy

import pytest
import torch
import torch.nn.functional as F

import __graft_entry__ as ge
from golden_util import elem_check, rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()


def maxnorm(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def fpn_weights(Cin, Cc, Cm, seed):
    g = torch.Generator().manual_seed(seed)
    w = {"lat": torch.randn(Cc, Cin, 1, 1, generator=g) / Cin ** 0.5, "lat_g": 1 + 0.1 * torch.randn(Cc, generator=g),
         "lat_b": 0.1 * torch.randn(Cc, generator=g), "out": torch.randn(Cc, Cc, 3, 3, generator=g) / (9 * Cc) ** 0.5,
         "out_g": 1 + 0.1 * torch.randn(Cc, generator=g), "out_b": 0.1 * torch.randn(Cc, generator=g)}
    if Cm:
        w["mask"] = torch.randn(Cm, Cc, 1, 1, generator=g) / Cc ** 0.5
        w["mask_b"] = 0.1 * torch.randn(Cm, generator=g)
    return w


def fpn_ref(x, up_nchw, w, groups=32):
    """float64 TL:313-324: GN(conv1x1(x)) + bilinear(up) -> ReLU(GN(conv3x3)) -> mask_feature conv1x1 + bias"""
    d = {k: v.double() for k, v in w.items()}
    lat = F.group_norm(F.conv2d(x.double(), d["lat"]), groups, d["lat_g"], d["lat_b"], 1e-5)
    m = lat + F.interpolate(up_nchw.double(), size=lat.shape[-2:], mode="bilinear", align_corners=False)
    c = F.relu(F.group_norm(F.conv2d(m, d["out"], padding=1), groups, d["out_g"], d["out_b"], 1e-5))
    mf = F.conv2d(c, d["mask"], d["mask_b"]) if "mask" in d else None
    return c, mf


def fpn_run(x, up_tok, Hu, Wu, w, Cm, want_y=True, groups=32):
    """one axvs_fpn_level_fwd call; up_tok: [N, Hu*Wu, C] fp32 token rows"""
    from axial_vs_amd import _lib
    L = _lib.lib()
    N, Cin, H, W = x.shape
    Cc = w["lat"].shape[0]
    dev = torch.device("cuda")
    dw = {k: v.float().contiguous().to(dev) for k, v in w.items()}
    ps = _lib.AxvsFpnLevelParams(dw["lat"].data_ptr(), dw["lat_g"].data_ptr(), dw["lat_b"].data_ptr(), dw["out"].data_ptr(), dw["out_g"].data_ptr(),
                                 dw["out_b"].data_ptr(), dw["mask"].data_ptr() if Cm else None, dw["mask_b"].data_ptr() if Cm else None)
    pk = torch.empty(L.axvs_fpn_level_packed_bytes(Cin, Cc, Cm), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(L.axvs_fpn_level_pack(C.byref(ps), pk.data_ptr(), Cin, Cc, Cm, 0, st), "pack")
    ws = torch.empty(L.axvs_fpn_level_workspace_bytes(N, H, W, Cin, Cc, groups), dtype=torch.uint8, device=dev)
    xd, ud = x.float().contiguous().to(dev), up_tok.float().contiguous().to(dev)
    y = torch.full((N, H * W, Cc), float("nan"), device=dev) if want_y else None
    mf = torch.full((N, Cm, H, W), float("nan"), device=dev) if Cm else None
    _lib.check(L.axvs_fpn_level_fwd(xd.data_ptr(), ud.data_ptr(), Hu * Wu * Cc, Cc, Hu, Wu, y.data_ptr() if y is not None else None,
                                    mf.data_ptr() if mf is not None else None, pk.data_ptr(), N, H, W, Cin, Cc, Cm, groups, 1e-5, 0,
                                    ws.data_ptr(), ws.numel(), st), "axvs_fpn_level_fwd")
    torch.cuda.synchronize()
    y = None if y is None else y.cpu().transpose(1, 2).reshape(N, Cc, H, W)
    return y, (None if mf is None else mf.cpu())


def case_inputs(N, Cin, Cc, H, W, Hu, Wu, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g)
    up = torch.randn(N, Cc, Hu, Wu, generator=g)
    return x, up, up.flatten(2).transpose(1, 2).contiguous()


@pytest.mark.parametrize("HW", [(1, 1), (3, 5), (7, 13), (25, 43), (96, 160)])
@pytest.mark.parametrize("Cin", [192, 256])
@pytest.mark.parametrize("N", [1, 5])
def test_fpn_conv3x3_gn_relu_against_float64(HW, Cin, N):
    H, W = HW
    Hu, Wu = (H + 1) // 2, (W + 1) // 2
    x, up, up_tok = case_inputs(N, Cin, 256, H, W, Hu, Wu, 100 + H + Cin + N)
    w = fpn_weights(Cin, 256, 256, 7 + Cin)
    c_ref, mf_ref = fpn_ref(x, up, w)
    y, mf = fpn_run(x, up_tok, Hu, Wu, w, 256)
    for name, a, b in (("c", y, c_ref), ("mask_feature", mf, mf_ref)):
        assert torch.isfinite(a).all(), name
        if H * W > 1:       # a 1 x 1 map: GroupNorm of 8 values per group, still checked below by max-norm
            elem_check(a, b, f"fpn {name} {N}x{Cin}x{H}x{W}")
        assert rel_l2(a, b) <= 1e-3 and maxnorm(a, b) <= 1e-3, (name, rel_l2(a, b), maxnorm(a, b))
    y2, mf2 = fpn_run(x, up_tok, Hu, Wu, w, 256)
    assert torch.equal(y, y2) and torch.equal(mf, mf2), "run-to-run bit identity"


@pytest.mark.parametrize("shape", [((25, 43), (13, 22)), ((7, 13), (5, 3)), ((12, 20), (12, 20)), ((9, 10), (4, 7)), ((5, 6), (11, 13))])
def test_fpn_bilinear_merge_ratios(shape):
    (H, W), (Hu, Wu) = shape
    x, up, up_tok = case_inputs(2, 256, 256, H, W, Hu, Wu, H * 31 + Hu)
    w = fpn_weights(256, 256, 0, 3)
    c_ref, _ = fpn_ref(x, up, w)
    y, _ = fpn_run(x, up_tok, Hu, Wu, w, 0)
    assert rel_l2(y, c_ref) <= 1e-3 and maxnorm(y, c_ref) <= 1e-3, (rel_l2(y, c_ref), maxnorm(y, c_ref))
    elem_check(y, c_ref, f"merge {shape}")


def test_ffn_pack_against_float64():
    from axial_vs_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(5)
    M, Cc, Fd = 777, 256, 1024
    x = torch.randn(M, Cc, generator=g)
    p = [1 + 0.1 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g), torch.randn(Fd, Cc, generator=g) / 16,
         0.1 * torch.randn(Fd, generator=g), torch.randn(Cc, Fd, generator=g) / 32, 0.1 * torch.randn(Cc, generator=g),
         1 + 0.1 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g)]
    d = [t.double() for t in p]
    y = F.layer_norm(x.double(), (Cc,), d[0], d[1], 1e-5)
    ref = F.layer_norm(y + F.linear(F.relu(F.linear(y, d[2], d[3])), d[4], d[5]), (Cc,), d[6], d[7], 1e-5)
    dp = [t.cuda().contiguous() for t in p]
    ps = _lib.AxvsFfnParams(*[t.data_ptr() for t in dp])
    st = torch.cuda.current_stream().cuda_stream
    pk = torch.empty(L.axvs_ffn_packed_bytes(Cc, Fd), dtype=torch.uint8, device="cuda")
    _lib.check(L.axvs_ffn_pack(C.byref(ps), pk.data_ptr(), Cc, Fd, 0, st), "axvs_ffn_pack")
    ws = torch.empty(L.axvs_ffn_workspace_bytes(M, Cc, Fd), dtype=torch.uint8, device="cuda")
    xd = x.cuda()
    out = torch.empty_like(xd)
    _lib.check(L.axvs_ffn_packed_fwd(xd.data_ptr(), out.data_ptr(), pk.data_ptr(), M, Cc, Fd, 0, ws.data_ptr(), ws.numel(), st), "axvs_ffn_packed_fwd")
    torch.cuda.synchronize()
    assert rel_l2(out.cpu(), ref) <= 1e-3 and maxnorm(out, ref) <= 1e-3
    elem_check(out.cpu(), ref, "ffn tail")


# ---------------------------------------------------------------------------------------------- module
def decoder_cfg(in_channels, num_layers, num_levels=3, num_temporal_levels=2):
    return dict(in_channels=in_channels, strides=[4, 8, 16, 32][:len(in_channels)], feat_channels=256, out_channels=256, num_outs=3,
                norm_cfg=dict(type="GN", num_groups=32), act_cfg=dict(type="ReLU"),
                encoder=dict(type="DetrTransformerEncoder", num_layers=num_layers, transformerlayers=dict(
                    type="BaseTransformerLayer", attn_cfgs=dict(type="MultiScaleDeformableAxialTrajectoryAttention", embed_dims=256, num_heads=8,
                                                                num_levels=num_levels, num_temporal_levels=num_temporal_levels, num_temporal_layers=1,
                                                                num_temporal_dim=1024, num_points=4, im2col_step=64, dropout=0.0, batch_first=False,
                                                                skip_connect=True, attn_drop=0.0, norm_cfg=None, init_cfg=None),
                    ffn_cfgs=dict(type="FFN", embed_dims=256, feedforward_channels=1024, num_fcs=2, ffn_drop=0.0, act_cfg=dict(type="ReLU", inplace=True)),
                    operation_order=("self_attn", "norm", "ffn", "norm")), init_cfg=None),
                positional_encoding=dict(type="SinePositionalEncoding", num_feats=128, normalize=True), init_cfg=None)


def make_decoder(in_channels=(64, 128, 192, 256), num_layers=2, seed=0, **kw):
    import axial_vs_amd as ax
    torch.manual_seed(seed)
    dec = ax.TubeLinkPixelDecoder(**decoder_cfg(list(in_channels), num_layers, **kw))
    with torch.no_grad():      # non-trivial GN affines, level / gamma values so that every term of the forward matters
        for n, p in dec.named_parameters():
            if n.endswith("gn.weight") or n.endswith("norms.0.weight") or n.endswith("norms.1.weight"):
                p.copy_(1 + 0.1 * torch.randn_like(p))
            elif n.endswith("gn.bias") or n.endswith("gamma") or "norms" in n:
                p.copy_(0.1 * torch.randn_like(p))
    return dec.cuda()


def feats_for(in_channels, BT, H4, W4, seed=1):
    g = torch.Generator().manual_seed(seed)
    out, h, w = [], H4, W4
    for c in in_channels:
        out.append(torch.randn(BT, c, h, w, generator=g).cuda())
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


def composition(dec, feats, T):
    """the same weights through the fp32 torch composition (the module's train-mode path, dropout 0)"""
    ref = copy.deepcopy(dec).train()
    with torch.no_grad():
        return ref(feats, T)


def check_outputs(got, want, tol=2e-3, contiguous=True):
    (mf, ms), (rmf, rms) = got, want
    assert len(ms) == len(rms)
    for a, b in [(mf, rmf)] + list(zip(ms, rms)):
        assert a.shape == b.shape and a.dtype == torch.float32 and (a.is_contiguous() or not contiguous)
        assert rel_l2(a, b) <= tol and maxnorm(a, b) <= 2 * tol, (tuple(a.shape), rel_l2(a, b), maxnorm(a, b))


@pytest.mark.parametrize("case", [dict(ch=(64, 128, 192, 256), T=2, hw=(32, 48), layers=2),
                                  dict(ch=(192, 384, 768, 1536), T=3, hw=(25, 43), layers=1, ntl=1)])
def test_module_eval_matches_composition(case):
    dec = make_decoder(case["ch"], case["layers"], num_temporal_levels=case.get("ntl", 2)).eval()
    feats = feats_for(case["ch"], case["T"], *case["hw"])
    with torch.no_grad():
        got = dec(feats, case["T"])
    check_outputs(got, composition(dec, feats, case["T"]))
    assert got[0].shape == (case["T"], 256) + case["hw"]
    assert [tuple(m.shape[-2:]) for m in got[1]][-1] == ((case["hw"][0] + 1) // 2, (case["hw"][1] + 1) // 2)


def test_two_fpn_levels_reference_indexing():
    """a 2-level encoder with equal in_channels: two FPN levels, lateral_convs[i] / output_convs[i] with the reference's loop index"""
    dec = make_decoder((256, 256, 256, 256), 1, num_levels=2, num_temporal_levels=1).eval()
    feats = feats_for((256,) * 4, 2, 24, 40)
    with torch.no_grad():
        got = dec(feats, 2)
    check_outputs(got, composition(dec, feats, 2))
    assert len(dec.lateral_convs) == 2 and len(got[1]) == 3


def test_per_clip_batch_matches_single_clips():
    dec = make_decoder().eval()
    f2 = feats_for((64, 128, 192, 256), 4, 16, 24, seed=3)
    with torch.no_grad():
        both = dec(f2, 2)
        one = dec([f[:2] for f in f2], 2)
        two = dec([f[2:] for f in f2], 2)
    for a, b, c in [(both[0], one[0], two[0])] + list(zip(both[1], one[1], two[1])):
        cat = torch.cat([b, c], 0)
        assert rel_l2(a, cat) <= 1e-5, rel_l2(a, cat)


def test_no_torch_compute_in_eval():
    dec = make_decoder().eval()
    feats = feats_for((64, 128, 192, 256), 2, 16, 24)
    with torch.no_grad():
        dec(feats, 2)
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
            dec(feats, 2)
            torch.cuda.synchronize()
    names = {e.key for e in prof.key_averages()}
    banned = {"aten::convolution", "aten::conv2d", "aten::group_norm", "aten::native_group_norm", "aten::upsample_bilinear2d",
              "aten::layer_norm", "aten::native_layer_norm", "aten::linear", "aten::addmm", "aten::mm", "aten::bmm"}
    assert not (names & banned), names & banned


def test_packs_track_parameter_updates():
    dec = make_decoder().eval()
    feats = feats_for((64, 128, 192, 256), 2, 16, 24)
    with torch.no_grad():
        before = dec(feats, 2)[0].clone()
        dec.output_convs[0].conv.weight.mul_(1.5)
        dec.encoder.layers[1].ffns[0].layers[1].weight.mul_(0.5)
        dec.mask_feature.bias.add_(0.25)
        after = dec(feats, 2)
    assert rel_l2(after[0], before) > 1e-2
    check_outputs(after, composition(dec, feats, 2))


def test_train_mode_runs_composition_with_gradients():
    dec = make_decoder(num_layers=1)
    feats = feats_for((64, 128, 192, 256), 2, 12, 16)
    dec.eval()
    with torch.no_grad():
        ev = dec(feats, 2)
    dec.train()
    mf, ms = dec(feats, 2)
    check_outputs((mf.detach(), [m.detach() for m in ms]), ev, contiguous=False)     # (the reference's views, as in TL:299-303)
    (mf.square().mean() + sum(m.mean() for m in ms)).backward()
    for n, p in dec.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
    # the FPN tail's gradients against float64 autograd of the same composition
    x = feats[0].detach().double().cpu().requires_grad_(True)
    up = ms[-1].detach().double().cpu()
    lat, out, mk = (copy.deepcopy(m).double().cpu() for m in (dec.lateral_convs[0], dec.output_convs[0], dec.mask_feature))
    y = out(lat(x) + F.interpolate(up, size=x.shape[-2:], mode="bilinear", align_corners=False))
    mk(y).square().mean().backward()
    for (n, p), (_, q) in zip(list(dec.lateral_convs[0].named_parameters()) + list(dec.output_convs[0].named_parameters()),
                              list(lat.named_parameters()) + list(out.named_parameters())):
        assert rel_l2(p.grad.cpu(), q.grad) <= 2e-3, (n, rel_l2(p.grad.cpu(), q.grad))


# ---------------------------------------------------------------------------------------------- against the reference's own decoder
G17 = ["g17_tl_pixdec_R50_B1_T2_32x48_l2", "g17_tl_pixdec_SwinL_B1_T3_25x43_l1", "g17_tl_pixdec_R50_B1_T4_48x80_l6"]


def g17_case(name):
    """decoder + inputs of a g17 fixture (tools/gen_golden_tl_pixel_decoder.py: the reference's MSDeformAttnPixelDecoder in float64)"""
    import numpy as np
    import axvs_oracle as orc
    import axial_vs_amd as ax
    from golden_util import load
    z, m = load(name)
    w = orc.random_weights(m["shapes"], m["seed"])
    w = {k: (v * 10.0 + 1.0 if k.endswith(".gamma") else v) for k, v in w.items()}       # the generator's O(1) gamma
    assert abs(sum(float(v.double().sum()) for v in w.values()) - float(z["wsum"])) < 1e-6 * abs(float(z["wsum"])), "torch RNG drift"
    cfg = decoder_cfg(m["in_channels"], m["layers"], num_temporal_levels=m["temporal_levels"])
    dec = ax.TubeLinkPixelDecoder(**cfg)
    dec.load_state_dict(w, strict=True)
    g = torch.Generator().manual_seed(m["seed"] + 1)
    feats = [torch.randn(m["B"] * m["T"], c, h, wd, generator=g, dtype=torch.float64) for c, (h, wd) in zip(m["in_channels"], m["sizes"])]
    for i, f in enumerate(feats):
        assert np.allclose([f.sum().item(), (f * f).sum().item(), f.abs().max().item()], z[f"feat{i}_checks"], rtol=1e-9)
    return z, m, dec.cuda().eval(), [f.float().cuda() for f in feats]


def g17_compare(z, key, got, rl2, mx):
    assert tuple(got.shape) == tuple(z[key + "_shape"]), (key, tuple(got.shape))
    a = got.reshape(-1)[::int(z[key + "_stride"])].double().cpu()
    b = torch.from_numpy(z[key])
    e_l2, e_mx = rel_l2(a, b), maxnorm(a, b)
    assert e_l2 <= rl2 and e_mx <= mx, (key, e_l2, e_mx)
    elem_check(a, b, key, tol=mx)
    return e_l2, e_mx


@pytest.mark.parametrize("name", G17)
def test_g17_end_to_end_against_reference(name):
    """f16 default: mask_feature and every multi_scale_features level against the reference decoder; 1e-3 on the 1 - 2 layer cases,
    1e-3 relative L2 / 1.5e-3 max-norm on the 6-layer stack (the within-clip stack's TOL_STACK rationale: six free-running layers of
    16-bit roundings); each encoder layer's output rows are checked on the way (free running, not teacher-forced)"""
    z, m, dec, feats = g17_case(name)
    mx = 1.5e-3 if m["layers"] >= 6 else 1e-3
    dec._record_layers = []
    with torch.no_grad():
        mf, ms = dec(feats, m["T"])
    layers, dec._record_layers = dec._record_layers, None
    torch.cuda.synchronize()
    errs = {"mask_feature": g17_compare(z, "mask_feature", mf, 1e-3, mx)}
    for i, x in enumerate(ms):
        errs[f"ms{i}"] = g17_compare(z, f"ms{i}", x, 1e-3, mx)
    assert len(layers) == m["layers"]
    for k, x in enumerate(layers):
        errs[f"layer{k}"] = g17_compare(z, f"layer{k}", x, 1e-3, mx)
    print(name, errs)
