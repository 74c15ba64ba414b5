"""GPU: every packed-weight site -- cache hit, rebuild after an in-place parameter update, rebuild after invalidate_pack -- at the
smallest size its pack function takes."""
import pytest
import torch

pytestmark = pytest.mark.gpu


class _Shape:
    def __init__(self, c, s):
        self.channels, self.stride = c, s


def _wc_decoder():
    import axial_vs_amd as ax
    return ax.WithinClipTrackingModule(
        {"res3": _Shape(32, 8), "res4": _Shape(64, 16), "res5": _Shape(64, 32)}, transformer_dropout=0.0, transformer_attn_drop=0.0, transformer_nheads=8,
        transformer_dim_feedforward=128, transformer_num_stages=1, transformer_spatial_layers=1, transformer_temporal_layers=1,
        transformer_temporal_attn_type="axial-trajectory", transformer_conv_dims=64, transformer_spatial_in_features=["res3", "res4", "res5"],
        transformer_temporal_in_features=["res4", "res5"], num_clip_frames=2, cross_clip_training=False).within_clip_tracking_module


def _tl_decoder():
    import axial_vs_amd as ax
    attn = dict(type="MultiScaleDeformableAxialTrajectoryAttention", embed_dims=256, num_heads=8, num_levels=2, num_temporal_levels=1,
                num_temporal_layers=1, num_temporal_dim=128, num_points=4)
    return ax.TubeLinkPixelDecoder(in_channels=[64, 64, 64, 64], encoder=dict(num_layers=1, transformerlayers=dict(
        attn_cfgs=attn, ffn_cfgs=dict(feedforward_channels=128, num_fcs=2), operation_order=("self_attn", "norm", "ffn", "norm"))))


def _cc_module(norm_fn):
    import axial_vs_amd as ax
    return ax.CrossClipTrackingModule(num_layers=1, num_classes=3, attn_drop=0.0, aspp_drop=0.0, kernel_sizes=[3, 3, 3], atrous_rates=[1, 2, 3],
                                      norm_fn=norm_fn, num_clip_frames=1)


def _site(kind):
    """(owner module, pack call, a parameter the blob holds)"""
    import axial_vs_amd as ax
    if kind == "traj_attn":
        m = ax.TrajectoryAttention(64, 8)
        return m, m._pack, m.proj_kv.weight
    if kind == "axial_layer":
        m = ax.TemporalAxialTrajectoryAttentionLayer(64, 128, n_heads=8)
        return m, m._pack, m.width_attn.q.weight
    if kind == "traj_layer":
        m = ax.TemporalTrajectoryAttentionLayer(64, 128, n_heads=8)
        return m, m._pack, m.linear2.weight
    if kind == "msda":
        m = ax.MSDeformAttn(64, 2, 8, 4)
        return m, m._pack, m.sampling_offsets.weight
    if kind == "msda_layer":
        m = ax.MSDeformAttnTransformerEncoderLayer(64, 128, n_levels=2, n_heads=8, n_points=4)
        return m, m._pack, m.self_attn.output_proj.weight
    if kind == "tl_plugin":
        m = ax.MultiScaleDeformableAxialTrajectoryAttention(embed_dims=64, num_levels=2, num_temporal_levels=1, num_temporal_dim=128)
        return m, m._pack, m.value_proj.weight
    if kind in ("cc_module", "cc_module_syncbn"):
        m = _cc_module("syncbn" if kind.endswith("syncbn") else "ln")
        return m, m._pack, m.conv_short_aggregate_layers[0]._proj_conv_bn_act.norm.weight
    if kind == "tl_cc_head":
        m = ax.TubeLinkCrossClipHead(num_classes=3, out_channels=128, num_cc_layers=1)
        return m, m._pack, m.mask_embed[2].weight
    if kind == "wc_decoder_projs":
        m = _wc_decoder()
        return m, m._pack_projs, m.output_proj[1][1].weight
    m = _tl_decoder()
    return {"tl_decoder_input": (m, lambda: m._pack_input(1), m.input_convs[1].gn.bias),
            "tl_decoder_ffn": (m, lambda: m._pack_ffn(0), m.encoder.layers[0].norms[1].weight),
            "tl_decoder_fpn_mask": (m, lambda: m._pack_fpn(0), m.mask_feature.weight),
            "tl_decoder_fpn": (m, lambda: m._pack_fpn(1), m.output_convs[1].conv.weight)}[kind]


def _bytes(blob) -> bytes:
    if isinstance(blob, torch.Tensor):
        return blob.cpu().numpy().tobytes()
    if isinstance(blob, (tuple, list)):
        return b"".join(_bytes(b) for b in blob)
    return repr(blob).encode()


@pytest.mark.parametrize("kind", ["traj_attn", "axial_layer", "traj_layer", "msda", "msda_layer", "tl_plugin", "cc_module", "cc_module_syncbn",
                                  "tl_cc_head", "wc_decoder_projs", "tl_decoder_input", "tl_decoder_ffn", "tl_decoder_fpn_mask", "tl_decoder_fpn"])
def test_pack_hits_tracks_in_place_updates_and_rebuilds_after_invalidate(kind):
    import axial_vs_amd as ax
    torch.manual_seed(3)
    owner, pack, param = _site(kind)
    owner.cuda().eval()
    first = pack()
    torch.cuda.synchronize()
    assert pack() is first                                   # hit: the stored object, nothing rebuilt
    before = _bytes(first)
    with torch.no_grad():
        param.add_(0.25)                                     # in place: same storage, new version
    updated = pack()
    torch.cuda.synchronize()
    assert updated is not first and pack() is updated
    after = _bytes(updated)
    assert len(after) == len(before) and after != before
    ax.invalidate_pack(owner)
    rebuilt = pack()
    torch.cuda.synchronize()
    assert rebuilt is not updated and _bytes(rebuilt) == after
    assert not any(k.startswith("_axvs") for k in owner.state_dict())
