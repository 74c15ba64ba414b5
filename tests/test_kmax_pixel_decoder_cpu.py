"""CPU: the restatement of Video-kMaX's pixel decoder (tests/kmax_pixel_decoder_cases.py) against fixtures of the reference's own
classes, the module's state-dict names, the head's child names, and the argument errors of the module and of the C-ABI
(axvs_kmax_pix_*), which are reported before any device work."""
import ctypes
import json
import os
import types

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import kmax_pixel_decoder_cases as pc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="session", autouse=True)
def built():
    ge.build()


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    m = json.loads(bytes(z["meta"]).decode())
    case = pc.Case(m["name"], m["seed"], tuple(m["spatial"]), m["N"], tuple(m["in_channels"]), tuple(m["dec_layers"]), tuple(m["dec_channels"]),
                   tuple(m["layer_types"]))
    return case, m, z


def check_against_fixture(z, outs, st, factor, what):
    """`outs` (name -> tensor) against the fixture's recorded values: within factor x the float32 restatement's own error against float64"""
    for k in pc.OUTPUTS:
        own = st["tol"][k] / 8
        if k in z.files:
            err = pc.err(outs[k], torch.from_numpy(z[k]))
        else:
            err = pc.err(outs[k][:, :, -1], torch.from_numpy(z[k + "_row"]))
            chk, t = z[k + "_checks"], outs[k].double().cpu()
            assert abs(chk[0] - float(t.sum())) <= factor * own * t.numel() and abs(chk[2] - float(t.abs().max())) <= factor * own, k
        print(f"{what} {k}: against the reference's fp32 run {err:.3e}, float32 restatement vs float64 {own:.3e}, bound {factor} x")
        assert err <= factor * own, k


def make_module(case):
    import axial_vs_amd as ax
    return ax.KMaXPixelDecoder(pc.input_shape(case), case.dec_layers, case.dec_channels, case.layer_types, case.spatial)


@pytest.mark.parametrize("fx", [c.name for c in pc.FIXTURES])
def test_restatement_reproduces_the_reference(fx):
    """The reference's own eval forward (fp32) against the float32 restatement on the same weights and inputs: every output within 8 x
    the float32 restatement's own error against float64; the key list is the fixture's."""
    case, m, z = load_fixture(fx)
    assert case == next(c for c in pc.FIXTURES if c.name == fx)
    assert m["keys"] == list(pc.param_shapes(case))
    st = pc.study(case)
    check_against_fixture(z, st["out32"], st, 8, fx)
    assert os.path.getsize(os.path.join(GOLDEN, fx + ".npz")) < 256 * 1024


def test_the_reference_order_needs_float32_weights():
    """Why the yardstick is a restatement: in float64 the reference's own op order has a softmax that casts to float, and the einsum
    behind it then meets float weights and double values."""
    w, v = torch.softmax(torch.randn(1, 8, 3, 3, dtype=torch.float64).float(), -1), torch.randn(1, 8, 4, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError):
        torch.einsum("bhlm,bhdm->bhdl", w, v)


@pytest.mark.parametrize("name", ["A", "C", "D"])
def test_state_dict_names(name):
    """The module carries the reference's own parameter and buffer names, in the reference's order (recorded in the fixtures from the
    reference's state_dict()), with the reference's shapes, `num_batches_tracked` included; a state under those names loads strictly."""
    case = pc.BY_NAME[name]
    mod = make_module(case)
    sd = mod.state_dict()
    assert list(sd) == list(pc.param_shapes(case))
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(pc.param_shapes(case))
    ck = pc.make_params(case)
    mod.load_state_dict(ck, strict=True)
    assert torch.equal(mod.state_dict()["_stages.1._blocks.0._attention._width_axis._value_rpe._embeddings.weight"],
                       ck["_stages.1._blocks.0._attention._width_axis._value_rpe._embeddings.weight"])


def test_shipped_configuration_size():
    mod = make_module(pc.BY_NAME["A"])
    assert len(mod.state_dict()) == 398
    assert sum(p.numel() for p in mod.parameters()) == 21151040


def test_fixture_names_are_the_modules():
    for fx in pc.FIXTURES:
        case, m, _ = load_fixture(fx.name)
        assert m["keys"] == list(make_module(case).state_dict())


def test_head_state_dict_prefixes():
    import axial_vs_amd as ax
    case = pc.BY_NAME["A"]
    predictor = ax.KMaXTransformerDecoder((1, 1, 1), (2048, 1024, 512), 4, 16, 2)
    head = ax.MaXTronDeepLabHead(None, make_module(case), predictor)
    assert {k.split(".")[0] for k in head.state_dict()} == {"pixel_decoder", "predictor"}
    assert [n for n, _ in head.named_children()] == ["pixel_decoder", "predictor"] and head.wc_module is None
    S = lambda c, s: types.SimpleNamespace(channels=c, stride=s)
    wc = ax.WithinClipTrackingModule(
        {"res3": S(32, 8), "res4": S(32, 16), "res5": S(32, 32)}, transformer_dropout=0.0, transformer_attn_drop=0.0, transformer_nheads=8,
        transformer_dim_feedforward=64, transformer_num_stages=1, transformer_spatial_layers=1, transformer_temporal_layers=1,
        transformer_temporal_attn_type="axial-trajectory", transformer_conv_dims=64, transformer_spatial_in_features=["res3", "res4", "res5"],
        transformer_temporal_in_features=["res3", "res4", "res5"], num_clip_frames=2, cross_clip_training=False)
    head = ax.MaXTronDeepLabHead(wc, make_module(case), predictor)
    assert [n for n, _ in head.named_children()] == ["wc_module", "pixel_decoder", "predictor"]
    assert {k.split(".")[0] for k in head.state_dict()} == {"wc_module", "pixel_decoder", "predictor"}


def test_train_mode_and_cpu_tensors_raise():
    case = pc.BY_NAME["B"]
    mod = make_module(case)
    feats = pc.make_inputs(case)
    with pytest.raises(NotImplementedError, match="forward-only"):
        mod.train().forward_features(feats)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        mod.eval().forward_features(feats)
    wrong = dict(feats, res4=feats["res4"][..., :-1])            # 4 x 5 where query_shape is 4 x 6
    with pytest.raises(NotImplementedError, match="must equal query_shape"):
        mod.forward_features(wrong)


S4 = dict(dec_layers=(1, 1, 1, 1), dec_channels=(512, 256, 128, 64), layer_types=("axial", "axial", "bottleneck", "bottleneck"))


@pytest.mark.parametrize("change, message", [
    (dict(dec_layers=(1, 1, 1), dec_channels=(512, 256, 128), layer_types=("axial", "axial", "bottleneck"), in_channels=(256, 512, 1024)), "four stages"),
    (dict(dec_channels=(384, 256, 128, 64)), "512, 256 or 128"),
    (dict(dec_channels=(512, 256, 128, 48)), "multiple of 32 up to 256"),
    (dict(dec_channels=(512, 256, 128, 288)), "multiple of 32 up to 256"),
    (dict(in_channels=(256, 512, 1024, 2056)), "multiples of 16 in 16..2048"),
    (dict(in_channels=(256, 512, 1024, 4096)), "multiples of 16 in 16..2048"),
    (dict(dec_layers=(1, 17, 1, 1)), "1..16 blocks"),
    (dict(dec_layers=(0, 1, 1, 1)), "1..16 blocks"),
    (dict(layer_types=("axial", "conv", "bottleneck", "bottleneck")), "neither"),
    (dict(spatial=(2593, 65)), "axis length 82"),                    # stride 32: 82 > 80 at base filter 512
    (dict(spatial=(65, 2081)), "axis length 131"),                   # stride 16: 131 > 128 at base filter 256
])
def test_configuration_bounds_raise(change, message):
    import axial_vs_amd as ax
    kw = dict(S4, in_channels=(256, 512, 1024, 2048), spatial=(65, 97))
    kw.update(change)
    shape = {f"res{5 - i}": types.SimpleNamespace(channels=c, stride=32 // 2 ** i) for i, c in enumerate(kw["in_channels"][::-1])}
    with pytest.raises(NotImplementedError, match=message):
        ax.KMaXPixelDecoder(shape, kw["dec_layers"], kw["dec_channels"], kw["layer_types"], kw["spatial"])


def test_axis_bound_follows_the_lds_plan():
    from axial_vs_amd.kmax_pixel_decoder import max_axis_length
    assert [max_axis_length(b) for b in (512, 256, 128)] == [80, 128, 128]        # the issue asks for 72 / 128 / 128 at least


def cfg_of(**kw):
    from axial_vs_amd import _lib
    i4 = ctypes.c_int * 4
    base = dict(N=1, in_channels=(2048, 1024, 512, 256), h=(3, 5, 9, 17), w=(4, 7, 13, 25), base=(512, 256, 128, 64), blocks=(1, 5, 1, 1),
                axial=(1, 1, 0, 0), heads=8)
    base.update(kw)
    return _lib.AxvsKpixCfg(**{k: (i4(*v) if isinstance(v, tuple) else v) for k, v in base.items()})


def test_library_exports_and_cabi_refusals():
    """The new entry points exist, and a configuration outside the bounds is refused before any device work: 0 bytes / AXVS_ERR_ARG with
    the bound in the message."""
    from axial_vs_amd import _lib
    L = _lib.lib()
    for name in ("axvs_kmax_pix_packed_bytes", "axvs_kmax_pix_pack", "axvs_kmax_pix_workspace_bytes", "axvs_kmax_pix_decoder_fwd",
                 "axvs_kmax_pix_axial_attn_fwd", "axvs_kmax_pix_block_fwd", "axvs_kmax_pix_fuse_fwd"):
        assert hasattr(L, name), name
    good = cfg_of()
    assert L.axvs_kmax_pix_packed_bytes(ctypes.byref(good)) > 21151040 * 4 * 0.9
    assert L.axvs_kmax_pix_workspace_bytes(ctypes.byref(good)) > 0
    for kw, message in [(dict(heads=4), "heads"), (dict(base=(384, 256, 128, 64)), "512, 256 or 128"), (dict(base=(512, 256, 128, 48)), "multiple of 32"),
                        (dict(h=(81, 5, 9, 17)), "axis length 81"), (dict(w=(4, 129, 13, 25)), "axis length 129"), (dict(blocks=(1, 17, 1, 1)), "blocks"),
                        (dict(in_channels=(2048, 1000, 512, 256)), "multiple of 16"), (dict(N=0), "frames"), (dict(h=(0, 5, 9, 17)), "pixels")]:
        bad = cfg_of(**kw)
        assert L.axvs_kmax_pix_packed_bytes(ctypes.byref(bad)) == 0, kw
        assert L.axvs_kmax_pix_workspace_bytes(ctypes.byref(bad)) == 0, kw
        assert message in L.axvs_last_error().decode(), (kw, L.axvs_last_error())
    rc = L.axvs_kmax_pix_decoder_fwd(ctypes.byref(cfg_of(h=(81, 5, 9, 17))), None, None, None, None, 0, None)
    assert rc == -1 and "axis length 81" in L.axvs_last_error().decode()
    assert L.axvs_kmax_pix_decoder_fwd(ctypes.byref(good), None, None, None, None, 0, None) == -1 and "null pointer" in L.axvs_last_error().decode()
    assert L.axvs_kmax_pix_block_fwd(ctypes.byref(good), None, 99, None, None, None, 0, None) == -1 and "block index" in L.axvs_last_error().decode()


def test_packed_slot_shapes_cover_the_folded_tensors():
    """_params.py's shape tables and its folding functions agree, slot by slot, on a block of either type and on a fuse without its
    high-resolution convolution."""
    from axial_vs_amd import _params as P
    case = pc.fuse_stage_case((3, 5), (5, 9), 128, 64, 64, 1)
    sd = pc.make_params(case)
    for prefix, cin, b, axial in (("_stages.0._blocks.0.", 16, 128, True), ("_stages.1._blocks.0.", 64, 64, False)):
        for (slot, shape), t in zip(P.kmax_pix_block_shapes(cin, b, axial), P.kmax_pix_block_folded(sd, prefix)):
            assert (shape is None) == (t is None) and (t is None or tuple(t.shape) == shape and t.dtype == torch.float64), slot
    for (slot, shape), t in zip(P.kmax_pix_fuse_shapes(512, 64, 64), P.kmax_pix_fuse_folded(sd, 0)):
        assert (shape is None) == (t is None) and (t is None or tuple(t.shape) == shape), slot
