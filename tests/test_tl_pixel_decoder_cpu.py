"""CPU: axial_vs_amd.TubeLinkPixelDecoder builds from the shipped Tube-Link pixel-decoder config dicts with the reference's state-dict
keys (mmcv 1.6.1 names), refuses what it has no HIP path for, and the new C-ABI entry points check their arguments."""
import ctypes as C

import pytest
import torch

import __graft_entry__ as ge


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()


class Attr(dict):
    """attribute-style dict (mmcv.ConfigDict stand-in)"""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


def attr(d):
    if isinstance(d, dict):
        return Attr({k: attr(v) for k, v in d.items()})
    return d


def cfg(in_channels=(256, 512, 1024, 2048), num_layers=6, attn_type="MultiScaleDeformableAxialTrajectoryAttention",
        order=("self_attn", "norm", "ffn", "norm"), act="ReLU", norm="GN"):
    """the pixel_decoder dict of configs/video/ovis/ovis_{r50,swin_l}_maxtron_*.py"""
    return dict(in_channels=list(in_channels), strides=[4, 8, 16, 32], feat_channels=256, out_channels=256, num_outs=3,
                norm_cfg=dict(type=norm, num_groups=32), act_cfg=dict(type="ReLU"),
                encoder=dict(type="DetrTransformerEncoder", num_layers=num_layers, transformerlayers=dict(
                    type="BaseTransformerLayer",
                    attn_cfgs=dict(type=attn_type, embed_dims=256, num_heads=8, num_levels=3, num_temporal_levels=2, num_temporal_layers=1,
                                   num_temporal_dim=1024, num_points=4, im2col_step=64, dropout=0.0, batch_first=False, skip_connect=True,
                                   attn_drop=0.1, norm_cfg=None, init_cfg=None),
                    ffn_cfgs=dict(type="FFN", embed_dims=256, feedforward_channels=1024, num_fcs=2, ffn_drop=0.0, act_cfg=dict(type=act, inplace=True)),
                    operation_order=order), init_cfg=None),
                positional_encoding=dict(type="SinePositionalEncoding", num_feats=128, normalize=True), init_cfg=None)


R50 = (256, 512, 1024, 2048)
SWIN_L = (192, 384, 768, 1536)


def expected_keys(in_channels, num_layers):
    """the reference decoder's state-dict under mmcv 1.6.1 (ConvModule conv/gn, BaseTransformerLayer attentions/ffns/norms)"""
    keys = {}
    for i, c in enumerate(reversed(in_channels[1:])):
        keys[f"input_convs.{i}.conv.weight"] = (256, c, 1, 1)
        keys[f"input_convs.{i}.conv.bias"] = (256,)
        keys[f"input_convs.{i}.gn.weight"] = keys[f"input_convs.{i}.gn.bias"] = (256,)
    for k in range(num_layers):
        a = f"encoder.layers.{k}.attentions.0."
        for n, s in (("sampling_offsets", (192, 256)), ("attention_weights", (96, 256)), ("value_proj", (256, 256)), ("output_proj", (256, 256))):
            keys[a + n + ".weight"], keys[a + n + ".bias"] = s, s[:1]
        keys[a + "gamma"] = (256,)
        f = f"encoder.layers.{k}.ffns.0.layers."
        keys[f + "0.0.weight"], keys[f + "0.0.bias"], keys[f + "1.weight"], keys[f + "1.bias"] = (1024, 256), (1024,), (256, 1024), (256,)
        for j in (0, 1):
            keys[f"encoder.layers.{k}.norms.{j}.weight"] = keys[f"encoder.layers.{k}.norms.{j}.bias"] = (256,)
    keys["level_encoding.weight"] = (3, 256)
    keys["level_3d_encodeing.weight"] = (2, 256)
    keys["lateral_convs.0.conv.weight"] = (256, in_channels[0], 1, 1)
    keys["lateral_convs.0.gn.weight"] = keys["lateral_convs.0.gn.bias"] = (256,)
    keys["output_convs.0.conv.weight"] = (256, 256, 3, 3)
    keys["output_convs.0.gn.weight"] = keys["output_convs.0.gn.bias"] = (256,)
    keys["mask_feature.weight"], keys["mask_feature.bias"] = (256, 256, 1, 1), (256,)
    return keys


@pytest.mark.parametrize("channels", [R50, SWIN_L])
@pytest.mark.parametrize("style", [dict, attr])
def test_builds_from_shipped_configs_with_reference_keys(channels, style):
    import axial_vs_amd as ax
    dec = ax.TubeLinkPixelDecoder(**style(cfg(channels, num_layers=2)))
    sd = dec.state_dict()
    exp = expected_keys(channels, 2)
    own = {k: tuple(v.shape) for k, v in sd.items() if ".attentions.0.temporal_layer." not in k}
    assert own == exp
    # the plugin is the existing module, reused as is
    assert isinstance(dec.encoder.layers[0].attentions[0], ax.MultiScaleDeformableAxialTrajectoryAttention)
    plugin_keys = {k for k in sd if ".attentions.0.temporal_layer." in k}
    assert plugin_keys == {f"encoder.layers.{k}.attentions.0.{n}" for k in range(2)
                           for n in ax.MultiScaleDeformableAxialTrajectoryAttention(num_levels=3).state_dict() if n.startswith("temporal_layer.")}
    dec2 = ax.TubeLinkPixelDecoder(**cfg(channels, num_layers=2))
    dec2.load_state_dict(sd, strict=True)
    assert dec.encoder.layers[0].attentions[0].batch_first is False


def test_init_weights_restates_reference():
    import axial_vs_amd as ax
    torch.manual_seed(0)
    dec = ax.TubeLinkPixelDecoder(**cfg(R50, num_layers=1))
    assert torch.all(dec.input_convs[0].conv.bias == 0) and torch.all(dec.mask_feature.bias == 0)
    # the trajectory plugin is NOT a MultiScaleDeformableAttention: after the xavier_normal_ sweep its offsets are not re-initialised
    assert dec.encoder.layers[0].attentions[0].sampling_offsets.weight.abs().sum() > 0
    assert dec.lateral_convs[0].conv.bias is None and dec.output_convs[0].conv.bias is None


@pytest.mark.parametrize("bad, field", [(dict(order=("norm", "self_attn", "norm", "ffn")), "operation_order"),
                                        (dict(attn_type="MultiScaleDeformableAttention"), "attn_cfgs.type"),
                                        (dict(act="GELU"), "act_cfg"), (dict(norm="BN"), "norm_cfg")])
def test_unsupported_configs_raise(bad, field):
    import axial_vs_amd as ax
    with pytest.raises(NotImplementedError, match=field.split(".")[-1]):
        ax.TubeLinkPixelDecoder(**cfg(**bad))


def test_fpn_and_ffn_entry_points_check_arguments():
    from axial_vs_amd import _lib
    L = _lib.lib()
    ERR_ARG, ERR_WS = -1, -2
    assert L.axvs_fpn_level_packed_bytes(256, 256, 256) > L.axvs_fpn_level_packed_bytes(256, 256, 0) > 0
    assert L.axvs_fpn_level_workspace_bytes(4, 96, 160, 256, 256, 32) > 4 * 96 * 160 * 256 * 4
    ps = _lib.AxvsFpnLevelParams(*([8] * 8))
    assert L.axvs_fpn_level_pack(None, 8, 256, 256, 256, 0, None) == ERR_ARG
    assert L.axvs_fpn_level_pack(C.byref(ps), 8, 200, 256, 256, 0, None) == ERR_ARG          # Cin not a multiple of 32
    assert L.axvs_fpn_level_pack(C.byref(ps), 8, 256, 250, 256, 0, None) == ERR_ARG          # C not a multiple of 32
    args = dict(x=16, up=16, ub=16 * 256, uld=256, Hu=4, Wu=4, y=16, mf=16, packed=16, N=1, H=8, W=8, Cin=256, Cc=256, Cm=256, groups=32)

    def call(ws_bytes=1 << 40, **kw):
        a = dict(args, **kw)
        return L.axvs_fpn_level_fwd(a["x"], a["up"], a["ub"], a["uld"], a["Hu"], a["Wu"], a["y"], a["mf"], a["packed"], a["N"], a["H"], a["W"],
                                    a["Cin"], a["Cc"], a["Cm"], a["groups"], 1e-5, 0, 16, ws_bytes, None)
    assert call(x=None) == ERR_ARG
    assert call(packed=None) == ERR_ARG
    assert call(y=None, mf=None) == ERR_ARG
    assert call(Cin=100) == ERR_ARG
    assert call(groups=24) == ERR_ARG                                         # groups must divide C
    assert call(H=0) == ERR_ARG
    assert call(Hu=0) == ERR_ARG
    assert call(uld=255) == ERR_ARG
    assert call(mf=16, Cm=0) == ERR_ARG
    assert call(N=1 << 16, H=1 << 8, W=1 << 8) == ERR_ARG                      # too many rows
    assert call(ws_bytes=1) == ERR_WS
    assert b"workspace" in L.axvs_last_error()
    # FFN tail
    fp = _lib.AxvsFfnParams(*([8] * 8))
    assert L.axvs_ffn_packed_bytes(256, 1024) > 0
    assert L.axvs_ffn_pack(None, 8, 256, 1024, 0, None) == ERR_ARG
    assert L.axvs_ffn_pack(C.byref(fp), 8, 256, 1000, 0, None) == ERR_ARG
    assert L.axvs_ffn_packed_fwd(None, 16, 16, 10, 256, 1024, 0, 16, 1 << 40, None) == ERR_ARG
    assert L.axvs_ffn_packed_fwd(16, 16, 16, 10, 250, 1024, 0, 16, 1 << 40, None) == ERR_ARG
    assert L.axvs_ffn_packed_fwd(16, 16, 16, 10, 256, 1024, 0, 16, 1, None) == ERR_WS
    assert L.axvs_fpn_level_fwd(16, 16, 4096, 256, 4, 4, 16, None, 16, 1, 8, 8, 256, 256, 0, 32, 1e-5, 7, 16, 1 << 40, None) == ERR_ARG   # dtype


G17 = ["g17_tl_pixdec_R50_B1_T2_32x48_l2", "g17_tl_pixdec_SwinL_B1_T3_25x43_l1", "g17_tl_pixdec_R50_B1_T4_48x80_l6"]


def g17_cfg(m):
    c = cfg(m["in_channels"], num_layers=m["layers"])
    c["encoder"]["transformerlayers"]["attn_cfgs"].update(num_temporal_levels=m["temporal_levels"], attn_drop=0.0)
    return c


@pytest.mark.parametrize("name", G17)
def test_state_dict_matches_reference_key_list(name):
    """key names, order-independent, and shapes equal those of the reference decoder stored in the g17 fixture
    (tools/gen_golden_tl_pixel_decoder.py); its weights load with strict=True"""
    import axial_vs_amd as ax
    from golden_util import load
    import axvs_oracle as orc
    z, m = load(name)
    dec = ax.TubeLinkPixelDecoder(**g17_cfg(m))
    sd = dec.state_dict()
    assert sorted(sd) == sorted(m["keys"])
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v) for k, v in m["shapes"].items()}
    dec.load_state_dict(orc.random_weights(m["shapes"], m["seed"]), strict=True)


def test_input_channels_checked_before_any_library_call():
    """two FPN levels with unequal in_channels: lateral_convs[1] is built for in_channels[0] and applied to feats[1] (the reference's
    indexing); like the reference's conv2d this is a shape error, raised before a pack sized for other channels is read"""
    import axial_vs_amd as ax
    c = cfg((256, 512, 1024, 2048), num_layers=1)
    c["encoder"]["transformerlayers"]["attn_cfgs"]["num_levels"] = 2
    c["encoder"]["transformerlayers"]["attn_cfgs"]["num_temporal_levels"] = 1
    dec = ax.TubeLinkPixelDecoder(**c).eval()
    feats = [torch.zeros(2, ch, 4, 4) for ch in (256, 512, 1024, 2048)]
    with pytest.raises(RuntimeError, match=r"lateral_convs\[1\] expects feats\[1\] with 256 channels"):
        dec(feats, 2)
    dec1 = ax.TubeLinkPixelDecoder(**cfg(SWIN_L, num_layers=1)).eval()
    with pytest.raises(RuntimeError, match=r"input_convs\[0\] expects feats\[3\] with 1536 channels"):
        dec1([torch.zeros(2, ch, 4, 4) for ch in (192, 384, 768, 2048)], 2)
    with pytest.raises(RuntimeError, match="expected 4 feature maps"):
        dec1([torch.zeros(2, ch, 4, 4) for ch in (192, 384, 768)], 2)
