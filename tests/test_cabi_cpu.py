"""CPU: the C-ABI library loads and exports every symbol include/axvs.h declares; host-side module surface."""
import ctypes
import os
import re

import pytest
import torch

import __graft_entry__ as ge
from golden_util import AXIAL, TRAJ, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="session", autouse=True)
def built():
    ge.build()


def header_symbols():
    text = open(os.path.join(ROOT, "include", "axvs.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(axvs_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from axial_vs_amd import _lib
    syms = header_symbols()
    assert len(syms) >= 10
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(raw, s), f"{s} declared in include/axvs.h but not exported"
    assert sorted(_lib.SIGNATURES) == syms, "ctypes prototypes out of sync with include/axvs.h"
    assert _lib.lib().axvs_version() >= 1


def test_size_queries_need_no_gpu():
    from axial_vs_amd import _lib
    L = _lib.lib()
    C, h, F = 256, 8, 1024
    packed = L.axvs_axial_layer_packed_bytes(C, h, F)
    # 2 x (7 C^2) 16-bit attention weights (+ 3 C^2 of per-head copies of the proj_kv halves for the reassociated temporal forms)
    # + 2 C F 16-bit FFN weights, plus fp32 biases / norms
    assert packed >= 2 * (2 * 10 * C * C) + 2 * (2 * C * F)
    assert packed < 1.1 * (2 * (2 * 10 * C * C) + 2 * (2 * C * F)) + 65536
    ws = L.axvs_axial_layer_workspace_bytes(1, 4, 64, 64, C, h, F)
    assert ws > 0
    assert L.axvs_traj_attn_workspace_bytes(4, 4, 16, C, h) > 0


def test_argument_errors_are_reported_not_raised_across_the_boundary():
    from axial_vs_amd import _lib
    L = _lib.lib()
    rc = L.axvs_axial_layer_fwd(None, None, None, None, 1, 4, 8, 8, 256, 8, 1024, 0, None, 0, None, None, None)
    assert rc == -1 and b"null" in L.axvs_last_error()
    rc = L.axvs_traj_pack(None, None, 250, 8, 0, None)
    assert rc == -1


@pytest.mark.parametrize("name", AXIAL[:2] + ["g4_encoder_B2_T2_C64_H6_W5"])
def test_state_dict_keys_match_reference(name):
    """strict load of a state dict with exactly the reference's parameter names and shapes."""
    import axial_vs_amd as ax
    import axvs_oracle as orc
    z, m = load(name)
    w = orc.random_weights(m["shapes"], 1)
    if "layers" in m:
        mod = ax.TemporalEncoder(m["C"], m["d_ffn"], n_heads=8, temporal_attn_type="axial-trajectory", num_temporal_layer=m["layers"])
    else:
        mod = ax.TemporalAxialTrajectoryAttentionLayer(m["C"], m["d_ffn"], n_heads=8)
    mod.load_state_dict(w, strict=True)
    assert set(mod.state_dict().keys()) == set(m["shapes"].keys())


def test_traj_state_dict_keys_match_reference():
    import axial_vs_amd as ax
    import axvs_oracle as orc
    z, m = load(TRAJ[0])
    mod = ax.TrajectoryAttention(m["C"], 8)
    mod.load_state_dict(orc.random_weights(m["shapes"], 1), strict=True)


def test_no_cpu_fallback_and_forward_only():
    import axial_vs_amd as ax
    layer = ax.TemporalAxialTrajectoryAttentionLayer(64, 128, n_heads=8)
    src, pos = torch.zeros(2, 12, 64), torch.zeros(1, 2, 3, 4, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer(src, pos)                       # training mode: the training tier (tests/test_hip_training.py), GPU only as well
    with pytest.raises(NotImplementedError):
        ax.TemporalTrajectoryAttentionLayer(64, 128, n_heads=8)(src, pos)     # the full T*H*W layer has no training tier
    layer.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer(src, pos)
    with pytest.raises(RuntimeError):
        ax.TemporalAxialTrajectoryAttentionLayer(64, 128, activation="swish")
    enc = ax.TemporalEncoder(64, 128, temporal_attn_type="axial_trajectory")   # the reference's default-string gotcha
    assert not hasattr(enc, "temporal_layers")
    full = ax.TemporalEncoder(64, 128, temporal_attn_type="trajectory", num_temporal_layer=1).eval()    # full T*H*W attention (a7)
    assert sorted(k for k in full.state_dict() if k.endswith(".q.weight")) == ["temporal_layers.0.temporal_attn.q.weight"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        full(src, pos)


@pytest.mark.parametrize("name", ["g5_cc_module_Q16_Tc3_V2_H8_L2", "g16_cc_module_syncbn_Q16_Tc3_V2_H8_L2"])
def test_cross_clip_state_dict_keys_match_reference(name):
    import axial_vs_amd as ax
    import axvs_oracle as orc
    z, m = load(name)
    mod = ax.CrossClipTrackingModule(num_layers=m["layers"], num_classes=m["num_classes"], attn_drop=0.0, aspp_drop=0.0,
                                     kernel_sizes=[3, 3, 3], atrous_rates=[1, 2, 3], norm_fn=m.get("norm_fn", "ln"), num_clip_frames=m["V"])
    ref_keys = set(m["shapes"].keys())
    own = {k: tuple(v.shape) for k, v in mod.state_dict().items() if v.dtype.is_floating_point}
    assert set(own.keys()) == ref_keys
    assert all(own[k] == m["shapes"][k] for k in ref_keys)
    sd = mod.state_dict()
    sd.update(orc.random_weights(m["shapes"], 1))
    mod.load_state_dict(sd, strict=True)


@pytest.mark.parametrize("name", ["g6_tl_cc_head_Tc3_Q16_f2_L2"])
def test_tube_link_head_state_dict_keys_match_reference(name):
    """TubeLinkCrossClipHead exposes the cross-clip members of the reference head under the reference's key names."""
    import axial_vs_amd as ax
    import axvs_oracle as orc
    z, m = load(name)
    mod = ax.TubeLinkCrossClipHead(num_classes=m["num_classes"], out_channels=m["Cm"], num_cc_layers=m["layers"])
    own = {k: tuple(v.shape) for k, v in mod.state_dict().items() if v.dtype.is_floating_point}
    assert set(own.keys()) == set(m["shapes"].keys())
    assert all(own[k] == tuple(m["shapes"][k]) for k in own)
    mod.load_state_dict(orc.random_weights(m["shapes"], 1), strict=True)
    with pytest.raises(RuntimeError):
        mod.eval()(torch.zeros(1, 3, 16, 256), torch.zeros(1, 6, m["Cm"], 8, 12))      # CPU tensors: no fallback


def test_msda_module_surface_matches_reference():
    """MSDeformAttn keeps the reference's parameter names / shapes / init (ops/modules/ms_deform_attn.py:59-79) and refuses
    CPU tensors (no fallback to a PyTorch sampling path)."""
    import axial_vs_amd as ax
    from golden_util import MSDA_MODULE
    z, m = load(MSDA_MODULE[0])
    mod = ax.MSDeformAttn(d_model=m["C"], n_levels=len(m["shapes"]), n_heads=m["M"], n_points=m["P"])
    own = {k: tuple(v.shape) for k, v in mod.state_dict().items()}
    assert own == {k: tuple(v) for k, v in m["wshapes"].items()}
    assert float(mod.sampling_offsets.weight.abs().max()) == 0.0 and float(mod.attention_weights.bias.abs().max()) == 0.0
    b = mod.sampling_offsets.bias.view(m["M"], len(m["shapes"]), m["P"], 2)
    assert torch.allclose(b[0, 0, :, 0], torch.arange(1, m["P"] + 1, dtype=torch.float32))     # head 0 points along +x, radius 1..P
    assert torch.allclose(b[:, :, 1], 2 * b[:, :, 0])
    with pytest.raises(RuntimeError):
        mod.eval()(torch.zeros(1, 4, m["C"]), torch.zeros(1, 4, len(m["shapes"]), 2), torch.zeros(1, 252, m["C"]), m["shapes"])


def _decoder_from_meta(m, cross_clip_training=False):
    import axial_vs_amd as ax

    class Shape:
        def __init__(self, c, s):
            self.channels, self.stride = c, s

    strides = {"res3": 8, "res4": 16, "res5": 32}
    return ax.WithinClipTrackingModule(
        {k: Shape(c, strides[k]) for k, c in m["chans"].items()}, transformer_dropout=0.0, transformer_attn_drop=0.0,
        transformer_nheads=8, transformer_dim_feedforward=m["d_ffn"], transformer_num_stages=m["stages"],
        transformer_spatial_layers=0 if m.get("temporal_only") else m["stages"], transformer_temporal_layers=m["stages"] * m["temporal_per_stage"],
        transformer_temporal_attn_type="axial-trajectory", transformer_conv_dims=256,
        transformer_spatial_in_features=["res3", "res4", "res5"], transformer_temporal_in_features=["res4", "res5"],
        num_clip_frames=m["T"], cross_clip_training=cross_clip_training)


def test_within_clip_module_state_dict_matches_reference():
    """WithinClipTrackingModule (pixel decoder: input/output projections, level embeddings, spatial + temporal stages) has the
    reference MSDeformAttnPixelDecoder's parameter names and shapes; CPU inputs raise."""
    import axvs_oracle as orc
    z, m = load("g8_pixel_decoder_T2_S2")
    mod = _decoder_from_meta(m)
    own = {k: tuple(v.shape) for k, v in mod.within_clip_tracking_module.state_dict().items()}
    assert own == {k: tuple(v) for k, v in m["shapes"].items()}
    mod.within_clip_tracking_module.load_state_dict(orc.random_weights(m["shapes"], 1), strict=True)
    with pytest.raises(RuntimeError):
        mod.eval().forward_features({k: torch.zeros(m["T"], c, *m["sizes"][k]) for k, c in m["chans"].items()})


def test_packed_weight_key_sees_replaced_parameters_and_modules():
    """The packed-weight cache key must change at once when a Parameter object is replaced by assignment, when it is updated
    in place, and when a whole submodule is replaced (the old key re-walked the module only every 256 calls)."""
    import axial_vs_amd as ax
    from axial_vs_amd.modules import _param_key
    layer = ax.TemporalAxialTrajectoryAttentionLayer(64, 128, n_heads=8)
    k0 = _param_key(layer, "f16")
    assert _param_key(layer, "f16") == k0 and _param_key(layer, "bf16") != k0
    layer.linear1.bias = torch.nn.Parameter(torch.zeros(128))                 # replaced Parameter object
    k1 = _param_key(layer, "f16")
    assert k1 != k0
    with torch.no_grad():
        layer.height_attn.q.weight.add_(1.0)                                  # in-place update (version counter)
    k2 = _param_key(layer, "f16")
    assert k2 != k1
    layer.norm2 = torch.nn.LayerNorm(64)                                      # replaced submodule
    k3 = _param_key(layer, "f16")
    assert k3 != k2 and _param_key(layer, "f16") == k3
    layer.load_state_dict(layer.state_dict())                                 # copy_ into the same Parameters
    assert _param_key(layer, "f16") != k3


def test_training_tier_has_no_cpu_fallback():
    """train() mode routes to the training tier, which refuses CPU tensors instead of falling back to torch."""
    import axial_vs_amd as ax
    import axvs_oracle as orc
    layer = ax.TemporalAxialTrajectoryAttentionLayer(64, 128, dropout=0.1, attn_drop=0.1, n_heads=8).train()
    src, pos = orc.synthetic_clip(1, 2, 64, 4, 4, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer(src, pos)
    from axial_vs_amd.training import layer_parameters
    names = [k for k, _ in layer.named_parameters()]
    assert len(layer_parameters(layer)) == len(names) == 32        # AxvsAxialLayerParams field order covers every parameter


def test_training_buffer_sizes_and_argument_checks():
    from axial_vs_amd import _lib
    L = _lib.lib()
    saved = L.axvs_axial_layer_train_saved_bytes(1, 4, 64, 64, 256, 8, 1024)
    M, C, T, F = 4 * 64 * 64, 256, 4, 1024
    assert saved >= 4 * (2 * (6 + 3 * T) * M * C + 4 * M * C + M * F)          # per pass q,k,v,xd,q2,o + x + kv2; pass outputs, z, u; r
    assert L.axvs_axial_layer_train_scratch_bytes(1, 4, 64, 64, 256, 8, 1024, 1) > L.axvs_axial_layer_train_scratch_bytes(1, 4, 64, 64, 256, 8, 1024, 0)
    assert L.axvs_axial_layer_train_saved_bytes(1, 4, 8, 8, 512, 4, 1024) == 0 and b"head_dim" in L.axvs_last_error()
    assert L.axvs_axial_layer_train_saved_bytes(1, 17, 8, 8, 256, 8, 1024) == 0 and b"T=17" in L.axvs_last_error()


def test_struct_fill_puts_each_pointer_in_its_field():
    """_lib.fill walks a parameter / gradient struct in declaration order (nested structs recursively, arrays element by element):
    pointer values 1..n land where the training tier's parameter lists put each tensor."""
    from axial_vs_amd import _lib
    traj = ["q_w", "q_b", "k_w", "k_b", "v_w", "v_b", "proj_q_w", "proj_q_b", "proj_kv_w", "proj_kv_b", "proj_w", "proj_b"]
    tail = ["norm1_w", "norm1_b", "linear1_w", "linear1_b", "linear2_w", "linear2_b", "norm2_w", "norm2_b"]
    msda = ["value_proj_w", "value_proj_b", "sampling_offsets_w", "sampling_offsets_b", "attention_weights_w", "attention_weights_b",
            "output_proj_w", "output_proj_b"]

    def expect(cls, paths):
        s = _lib.fill(cls, range(1, len(paths) + 1))
        for v, path in enumerate(paths, 1):
            obj = s
            for part in path.split("."):
                obj = obj[int(part)] if part.isdigit() else getattr(obj, part)
            assert obj == v, (cls.__name__, path, obj, v)
        with pytest.raises(ValueError):
            _lib.fill(cls, range(1, len(paths) + 2))
        return s

    s = expect(_lib.AxvsAxialLayerParams, [f"height_attn.{n}" for n in traj] + [f"width_attn.{n}" for n in traj] + tail)
    assert s.width_attn.q_w == 13 and s.norm2_b == 32
    expect(_lib.AxvsTrajLayerParams, [f"temporal_attn.{n}" for n in traj] + tail)
    expect(_lib.AxvsMsdaLayerParams, [f"self_attn.{n}" for n in msda] + tail)
    s = expect(_lib.AxvsTLHeadParams, ["post_norm_w", "post_norm_b", "activation_proj_w", "activation_proj_b", "cls_embed_w", "cls_embed_b",
                                       "mask_embed_w.0", "mask_embed_w.1", "mask_embed_w.2", "mask_embed_b.0", "mask_embed_b.1", "mask_embed_b.2"])
    assert list(s.mask_embed_w) == [7, 8, 9] and list(s.mask_embed_b) == [10, 11, 12]
    expect(_lib.AxvsCCHeadGrads, ["class_proj_w", "class_proj_bn.w", "class_proj_bn.b", "mask_proj_w", "mask_proj_bn.w", "mask_proj_bn.b",
                                  "mask_head_w", "mask_head_bn.w", "mask_head_bn.b", "class_head_w", "class_head_b", "act_head_w",
                                  "act_head_b", "pixel_bn.w", "pixel_bn.b"])


def test_cross_clip_module_parameters_are_the_chain_then_the_heads():
    import axial_vs_amd as ax
    from axial_vs_amd.cc_training import chain_parameters, module_parameters
    nl = 2
    mod = ax.CrossClipTrackingModule(num_layers=nl, num_classes=3, attn_drop=0.0, aspp_drop=0.0, kernel_sizes=[3, 3, 3], atrous_rates=[1, 2, 3],
                                     norm_fn="ln", num_clip_frames=1)
    ps = module_parameters(mod)
    assert len(ps) == nl * 21 + 15
    assert all(a is b for a, b in zip(ps, chain_parameters(mod, nl)))
    assert len({id(p) for p in ps}) == len(ps)


def _field_paths(cls, prefix=""):
    """dotted paths of a parameter struct's pointer slots in declaration order (nested structs recursively, arrays by element)"""
    out = []
    for name, t in cls._fields_:
        if issubclass(t, ctypes.Structure):
            out += _field_paths(t, prefix + name + ".")
        elif issubclass(t, ctypes.Array):
            out += [f"{prefix}{name}.{k}" for k in range(t._length_)]
        else:
            out.append(prefix + name)
    return out


def _by_path(mod, path):
    """the tensor a field path names on a module whose attributes the struct's fields follow: `a.b_w` -> mod.a.b.weight"""
    *owners, leaf = path.split(".")
    for o in owners:
        mod = getattr(mod, o)
    attr, kind = leaf.rsplit("_", 1)
    return getattr(getattr(mod, attr), {"w": "weight", "b": "bias"}[kind])


def _tl_decoder(num_layers=1):
    import axial_vs_amd as ax
    attn = dict(type="MultiScaleDeformableAxialTrajectoryAttention", embed_dims=256, num_heads=8, num_levels=2, num_temporal_levels=1,
                num_temporal_layers=1, num_temporal_dim=128, num_points=4)
    return ax.TubeLinkPixelDecoder(in_channels=[64, 64, 64, 64], encoder=dict(num_layers=num_layers, transformerlayers=dict(
        attn_cfgs=attn, ffn_cfgs=dict(feedforward_channels=128, num_fcs=2), operation_order=("self_attn", "norm", "ffn", "norm"))))


def _cc_module(nl=1, norm_fn="ln"):
    import axial_vs_amd as ax
    return ax.CrossClipTrackingModule(num_layers=nl, num_classes=3, attn_drop=0.0, aspp_drop=0.0, kernel_sizes=[3, 3, 3], atrous_rates=[1, 2, 3],
                                      norm_fn=norm_fn, num_clip_frames=1)


def _same(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a is b, i


def _fill_takes_exactly(cls, n):
    from axial_vs_amd import _lib
    _lib.fill(cls, range(1, n + 1))
    for wrong in (n - 1, n + 1):
        with pytest.raises(ValueError):
            _lib.fill(cls, range(1, wrong + 1))


def test_order_functions_name_each_struct_field_in_declaration_order():
    """Every function of axial_vs_amd._params returns, slot by slot, the very Parameter its struct's field names -- and as many as
    _lib.fill takes for that struct."""
    import axial_vs_amd as ax
    from axial_vs_amd import _lib, _params as P
    from axial_vs_amd.pixel_decoder import _conv_gn
    # structs whose fields follow the module's attribute names: the expected tensor comes from the field path
    attn = ax.TrajectoryAttention(64, 8)
    msda = ax.MSDeformAttn(64, 2, 8, 4)
    plugin = ax.MultiScaleDeformableAxialTrajectoryAttention(embed_dims=64, num_levels=2, num_temporal_dim=128)
    for cls, fn, mod in ((_lib.AxvsTrajParams, P.traj_params, attn),
                         (_lib.AxvsAxialLayerParams, P.axial_layer_params, ax.TemporalAxialTrajectoryAttentionLayer(64, 128, n_heads=8)),
                         (_lib.AxvsTrajLayerParams, P.traj_layer_params, ax.TemporalTrajectoryAttentionLayer(64, 128, n_heads=8)),
                         (_lib.AxvsMsdaParams, P.msda_params, msda), (_lib.AxvsMsdaParams, P.msda_params, plugin),
                         (_lib.AxvsMsdaLayerParams, P.msda_layer_params, ax.MSDeformAttnTransformerEncoderLayer(64, 128, n_levels=2, n_heads=8, n_points=4))):
        paths = _field_paths(cls)
        _same(fn(mod), [_by_path(mod, p) for p in paths])
        _fill_takes_exactly(cls, len(paths))
    # the others: the expected attributes, spelled out here
    pair = _conv_gn(32, 64)
    _same(P.conv_gn_params(pair[0], pair[1]), [pair[0].weight, pair[0].bias, pair[1].weight, pair[1].bias])
    dec = _tl_decoder()
    cm = dec.input_convs[0]
    _same(P.conv_gn_params(cm.conv, cm.gn), [cm.conv.weight, cm.conv.bias, cm.gn.weight, cm.gn.bias])
    _fill_takes_exactly(_lib.AxvsConvGnParams, 4)
    lay = dec.encoder.layers[0]
    _same(P.ffn_params(lay), [lay.norms[0].weight, lay.norms[0].bias, lay.ffns[0].layers[0][0].weight, lay.ffns[0].layers[0][0].bias,
                              lay.ffns[0].layers[1].weight, lay.ffns[0].layers[1].bias, lay.norms[1].weight, lay.norms[1].bias])
    assert _field_paths(_lib.AxvsFfnParams) == ["norm1_w", "norm1_b", "linear1_w", "linear1_b", "linear2_w", "linear2_b", "norm2_w", "norm2_b"]
    _fill_takes_exactly(_lib.AxvsFfnParams, 8)
    assert len(dec.lateral_convs) == 2
    for i, mask in ((0, dec.mask_feature), (1, None)):
        lat, out = dec.lateral_convs[i], dec.output_convs[i]
        _same(P.fpn_level_params(lat, out, mask), [lat.conv.weight, lat.gn.weight, lat.gn.bias, out.conv.weight, out.gn.weight, out.gn.bias,
                                                   None if mask is None else mask.weight, None if mask is None else mask.bias])
    assert _field_paths(_lib.AxvsFpnLevelParams) == ["lateral_w", "lateral_gn_w", "lateral_gn_b", "output_w", "output_gn_w", "output_gn_b", "mask_w", "mask_b"]
    _fill_takes_exactly(_lib.AxvsFpnLevelParams, 8)
    s = _lib.fill(_lib.AxvsFpnLevelParams, [1, 2, 3, 4, 5, 6, None, None])
    assert s.mask_w is None and s.mask_b is None and s.output_gn_b == 6

    # cross-clip layer: 21 tensors (fused qkv) for 25 slots; cc_layer_struct places the q / k / v row blocks of the fused projection
    mod = _cc_module(nl=2)
    for i in range(2):
        lay, asp, cn = mod.transformer_trajectory_self_attention_layers[i], mod.conv_short_aggregate_layers[i], mod.conv_norms[i]
        at, pj = lay.self_attn, asp._proj_conv_bn_act
        want = {"attn.q_w": (at.qkv.weight, 0), "attn.q_b": (at.qkv.bias, 0), "attn.k_w": (at.qkv.weight, 4 * 256 * 256), "attn.k_b": (at.qkv.bias, 4 * 256),
                "attn.v_w": (at.qkv.weight, 8 * 256 * 256), "attn.v_b": (at.qkv.bias, 8 * 256), "attn.proj_q_w": (at.proj_q.weight, 0),
                "attn.proj_q_b": (at.proj_q.bias, 0), "attn.proj_kv_w": (at.proj_kv.weight, 0), "attn.proj_kv_b": (at.proj_kv.bias, 0),
                "attn.proj_w": (at.proj.weight, 0), "attn.proj_b": (at.proj.bias, 0), "norm_w": (lay.norm.weight, 0), "norm_b": (lay.norm.bias, 0),
                "aspp_w.0": (asp._aspp_conv0.weight, 0), "aspp_w.1": (asp._aspp_conv1.weight, 0), "aspp_w.2": (asp._aspp_conv2.weight, 0),
                "aspp_b.0": (asp._aspp_conv0.bias, 0), "aspp_b.1": (asp._aspp_conv1.bias, 0), "aspp_b.2": (asp._aspp_conv2.bias, 0),
                "aspp_proj_w": (pj.conv.weight, 0), "aspp_norm_w": (pj.norm.weight, 0), "aspp_norm_b": (pj.norm.bias, 0),
                "conv_norm_w": (cn.weight, 0), "conv_norm_b": (cn.bias, 0)}
        ps = P.cc_layer_params(mod, i)
        assert len(ps) == P.CC_PER_LAYER == 21 and len({id(t) for t in ps}) == 21
        st = P.cc_layer_struct([(k + 1) << 32 for k in range(21)])          # (entry k as a fake address with room for the offsets)
        paths = _field_paths(_lib.AxvsCCLayerParams)
        assert sorted(paths) == sorted(want)
        for path in paths:
            v = st
            for part in path.split("."):
                v = v[int(part)] if part.isdigit() else getattr(v, part)
            assert ps[(v >> 32) - 1] is want[path][0] and v & 0xffffffff == want[path][1], path
        _same(P.cc_chain_params(mod, 2)[21 * i:21 * (i + 1)], ps)
    for wrong in (20, 22):
        with pytest.raises(ValueError):
            P.cc_layer_struct(list(range(1, wrong + 1)))
    # cross-clip heads: the trainable tensors in AxvsCCHeadGrads order; with the running statistics, AxvsCCHeadParams order
    pr, cp, mp = mod._predictor, mod._class_embedding_projection, mod._mask_embedding_projection
    want = {"class_proj_w": cp.conv.weight, "class_proj_bn": cp.norm, "mask_proj_w": mp.conv.weight, "mask_proj_bn": mp.norm,
            "mask_head_w": pr._transformer_mask_head.conv.weight, "mask_head_bn": pr._transformer_mask_head.norm,
            "class_head_w": pr._transformer_class_head.conv.weight, "class_head_b": pr._transformer_class_head.conv.bias,
            "act_head_w": pr._transformer_class_activation_head.conv.weight, "act_head_b": pr._transformer_class_activation_head.conv.bias,
            "pixel_bn": pr._pixel_space_mask_batch_norm}
    bn_attr = {"w": "weight", "b": "bias", "mean": "running_mean", "var": "running_var"}

    def head_tensor(path):
        name, _, sub = path.partition(".")
        return getattr(want[name], bn_attr[sub]) if sub else want[name]
    heads = P.cc_head_params(mod)
    _same(heads, [head_tensor(p) for p in _field_paths(_lib.AxvsCCHeadGrads)])
    _fill_takes_exactly(_lib.AxvsCCHeadGrads, 15)
    running = [(bn.running_mean, bn.running_var) for bn in P.cc_bn_modules(mod)]
    _same(P.cc_head_with_running(heads, running), [head_tensor(p) for p in _field_paths(_lib.AxvsCCHeadParams)])
    _fill_takes_exactly(_lib.AxvsCCHeadParams, 23)
    _same(P.cc_module_params(mod), P.cc_chain_params(mod, 2) + heads)
    # Tube-Link head
    hd = ax.TubeLinkCrossClipHead(num_classes=3, out_channels=128, num_cc_layers=1)
    pn, me = hd.transformer_decoder.post_norm, hd.mask_embed
    _same(P.tl_head_params(hd), [pn.weight, pn.bias, hd.activation_proj.weight, hd.activation_proj.bias, hd.cls_embed.weight, hd.cls_embed.bias,
                                 me[0].weight, me[2].weight, me[4].weight, me[0].bias, me[2].bias, me[4].bias])
    assert _field_paths(_lib.AxvsTLHeadParams) == ["post_norm_w", "post_norm_b", "activation_proj_w", "activation_proj_b", "cls_embed_w", "cls_embed_b",
                                                   "mask_embed_w.0", "mask_embed_w.1", "mask_embed_w.2", "mask_embed_b.0", "mask_embed_b.1", "mask_embed_b.2"]
    _fill_takes_exactly(_lib.AxvsTLHeadParams, 12)


def test_training_tier_hands_autograd_the_order_functions_tensors(monkeypatch):
    """What each training entry point passes to its autograd Function as parameters is, element for element, what the struct's order
    function returns (the Parameters themselves: autograd accumulates into their .grad)."""
    import axial_vs_amd as ax
    from axial_vs_amd import _params as P, cc_training, glue_training, training
    from axial_vs_amd.pixel_decoder import _conv_gn

    class Handed(Exception):
        pass

    def record(owner, fn, *args):
        raise Handed(args)

    def handed(call, *args, **kw):
        with pytest.raises(Handed) as e:
            call(*args, **kw)
        return e.value.args[0]

    monkeypatch.setattr(training, "apply", record)
    monkeypatch.setattr(cc_training, "apply", record)
    monkeypatch.setattr(glue_training._ConvGnTrain, "apply", staticmethod(lambda *args: record(None, None, *args)))
    src, pos = torch.zeros(2, 12, 64), torch.zeros(1, 2, 3, 4, 64)
    layer = ax.TemporalAxialTrajectoryAttentionLayer(64, 128, n_heads=8)
    want = P.axial_layer_params(layer)
    assert len(want) == 32
    _same(handed(training.axial_layer_train, layer, src, pos)[-32:], want)
    _same(training.layer_parameters(layer), want)
    layer = ax.TemporalTrajectoryAttentionLayer(64, 128, n_heads=8)
    _same(handed(training.traj_layer_train, layer, src, pos)[-20:], P.traj_layer_params(layer))
    _same(training.traj_layer_parameters(layer), P.traj_layer_params(layer))
    layer = ax.MSDeformAttnTransformerEncoderLayer(64, 128, n_levels=1, n_heads=8, n_points=4)
    _same(handed(training.msda_layer_train, layer, torch.zeros(1, 12, 64), None, torch.zeros(1, 12, 1, 2), [(3, 4)])[-16:], P.msda_layer_params(layer))
    nl = 2
    mod = _cc_module(nl)
    want = P.cc_module_params(mod)
    assert len(want) == nl * 21 + 15
    _same(handed(cc_training.cc_module_train, mod, torch.zeros(1, 16, 2, 256), torch.zeros(1, 128, 2, 4, 8))[-len(want):], want)
    _same(cc_training.module_parameters(mod), want)
    _same(cc_training.chain_parameters(mod, nl), want[:nl * 21])
    _same(handed(cc_training.cc_layers_train, mod, torch.zeros(1, 16, 2, 256), nl, [1, 2, 3], 0.0, 0.0)[-nl * 21:], P.cc_chain_params(mod, nl))
    hd = ax.TubeLinkCrossClipHead(num_classes=3, out_channels=128, num_cc_layers=1)
    cfg = cc_training.tl_heads_cfg(1, 1, 16, 2, 1, 4, 8, 4, 128)
    _same(handed(cc_training.tl_heads_train, hd, torch.zeros(1, 1, 16, 2, 256), torch.zeros(1, 2, 128, 4, 8), cfg)[-12:], P.tl_head_params(hd))
    _same(cc_training.tl_heads_parameters(hd), P.tl_head_params(hd))
    pair = _conv_gn(32, 64)
    _same(handed(glue_training.conv_gn_train, torch.zeros(1, 32, 3, 4), pair[0], pair[1])[1:5], P.conv_gn_params(pair[0], pair[1]))


def test_invalidate_pack_clears_every_stored_blob():
    """Every pack site keeps its blobs in the same slot of its owner's __dict__ (not a buffer: state dicts do not see it);
    invalidate_pack empties that slot on a module and on all its children -- both pixel decoders included."""
    import axial_vs_amd as ax
    from axial_vs_amd import modules
    z, m = load("g8_pixel_decoder_T2_S2")
    wc = _decoder_from_meta(m)
    owners = [ax.TrajectoryAttention(64, 8), ax.TemporalAxialTrajectoryAttentionLayer(64, 128, n_heads=8),
              ax.TemporalTrajectoryAttentionLayer(64, 128, n_heads=8), ax.MSDeformAttn(64, 2, 8, 4),
              ax.MSDeformAttnTransformerEncoderLayer(64, 128, n_levels=2, n_heads=8, n_points=4),
              ax.MultiScaleDeformableAxialTrajectoryAttention(embed_dims=64, num_levels=2, num_temporal_dim=128), _cc_module(),
              ax.TubeLinkCrossClipHead(num_classes=3, out_channels=128, num_cc_layers=1), wc.within_clip_tracking_module, _tl_decoder()]
    sentinel = object()
    keys_before = [set(o.state_dict()) for o in owners]
    for o in owners:
        o.__dict__[modules._PACKS] = {"slot": ("key", sentinel), "other": ("key", sentinel)}
    assert [set(o.state_dict()) for o in owners] == keys_before
    parent = torch.nn.ModuleList([torch.nn.ModuleList(owners[:5]), *owners[5:-1], wc])       # (the within-clip decoder as a grandchild)
    ax.invalidate_pack(parent)
    ax.invalidate_pack(owners[-1])
    for o in owners:
        assert modules._PACKS not in o.__dict__, type(o).__name__
        assert not any(v is sentinel for v in o.__dict__.values())


def test_reference_extension_stand_in_exposes_the_two_entry_points():
    """`import MultiScaleDeformableAttention as MSDA` (OPS/functions/ms_deform_attn_func.py:22) resolves to the stand-in module and
    finds ms_deform_attn_forward / ms_deform_attn_backward with the extension's argument lists (OPS/src/ms_deform_attn.h:24-67)."""
    import importlib
    import inspect
    import sys
    import axial_vs_amd
    sys.path.insert(0, os.path.join(os.path.dirname(axial_vs_amd.__file__), "compat"))
    try:
        MSDA = importlib.import_module("MultiScaleDeformableAttention")
    finally:
        sys.path.pop(0)
    f = list(inspect.signature(MSDA.ms_deform_attn_forward).parameters)
    b = list(inspect.signature(MSDA.ms_deform_attn_backward).parameters)
    assert f == ["value", "value_spatial_shapes", "value_level_start_index", "sampling_locations", "attention_weights", "im2col_step"]
    assert b == ["value", "value_spatial_shapes", "value_level_start_index", "sampling_locations", "attention_weights", "grad_output", "im2col_step"]


def test_default_dtype_f32_falls_back_to_16_bit_where_there_is_no_fp32_tier():
    """`set_default_dtype("f32")` selects the fp32 tier of the axial layer; modules without such a tier (TrajectoryAttention, the
    cross-clip module, deformable attention, ...) keep 16-bit operands instead of failing on an unknown dtype (round-3 advisor)."""
    import axial_vs_amd as ax
    from axial_vs_amd import modules
    prev = modules._DEFAULT_DTYPE
    try:
        modules.set_default_dtype("f32")
        assert modules.default_operand_dtype() == "f16"
        assert ax.TrajectoryAttention(64, 8)._dtype() == "f16"
        layer = ax.TemporalAxialTrajectoryAttentionLayer(64, 128, n_heads=8)
        assert layer._dtype() == "f32"
        with pytest.raises(NotImplementedError):
            layer._pack()                      # the fp32 tier has no packed weights / per-pass entry point
        modules.set_default_dtype("bf16")
        assert modules.default_operand_dtype() == "bf16" and layer._dtype() == "bf16"
        with pytest.raises(ValueError):
            modules.set_default_dtype("fp8")
    finally:
        modules.set_default_dtype(prev)


def test_stack_precision_setter_reaches_every_axial_layer():
    """`WithinClipTrackingModule.set_stack_precision`: the operand precision of the axial-trajectory layers of the stack (the fp32
    setting is what holds 1e-3 in max-norm over the free-running stack of BASELINE config 3; GPU test
    test_within_clip_module_full_size_fp32_stack_holds_the_bar_in_max_norm)."""
    import axial_vs_amd as ax
    z, m = load("g8_pixel_decoder_T2_S2")
    mod = _decoder_from_meta(m)
    layers = [x for x in mod.modules() if isinstance(x, ax.TemporalAxialTrajectoryAttentionLayer)]
    assert layers and all(l.mfma_dtype is None for l in layers)
    assert mod.set_stack_precision("f32") is mod and all(l._dtype() == "f32" for l in layers)
    mod.set_stack_precision("f16")
    assert all(l._dtype() == "f16" for l in layers)
    with pytest.raises(ValueError):
        mod.set_stack_precision("fp8")


def test_forward_hooks_keep_the_split_and_cat_data_flow():
    """The decoder's eval path runs the temporal levels in place in the token buffer, bypassing `TemporalEncoder.forward()`; a
    module with forward (pre-)hooks must keep the reference's data flow, where the hooks see the per-level tensors."""
    import axial_vs_amd as ax
    from axial_vs_amd.modules import _has_hooks
    enc = ax.TemporalEncoder(256, 1024, temporal_attn_type="axial-trajectory", num_temporal_layer=2).eval()
    assert not _has_hooks(enc) and not any(_has_hooks(l) for l in enc.temporal_layers)
    h = enc.register_forward_hook(lambda m, a, o: None)
    assert _has_hooks(enc) and not enc.can_run_in_place(torch.zeros(1, 2, 4, 4, 256))
    h.remove()
    assert not _has_hooks(enc)
    h = enc.temporal_layers[1].register_forward_pre_hook(lambda m, a: None)
    assert _has_hooks(enc.temporal_layers[1])
    h.remove()
    assert not enc.train().can_run_in_place(torch.zeros(1, 2, 4, 4, 256))      # train() mode: autograd needs the out-of-place path


def test_status_check_and_state_error_are_part_of_the_abi():
    """Round 5: AXVS_ERR_STATE / axvs_check_status / option sync_spin_limit exist; without a registered word the check passes, and
    registering NULL (no GPU call involved) keeps it that way."""
    from axial_vs_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "axvs.h")).read()
    assert "#define AXVS_ERR_STATE (-4)" in hdr and _lib.ERR_STATE == -4
    assert L.axvs_set_status_buffer(None) == 0
    assert L.axvs_check_status() == 0
    assert L.axvs_set_option(b"sync_spin_limit", 1000) == 0 and L.axvs_set_option(b"sync_spin_limit", 0) == 0


def test_train_amp_context_releases_its_lock_when_the_option_call_fails(monkeypatch):
    """advisor (round 4): __enter__ took the lock and set the mode before a failing option call; __exit__ never ran."""
    from axial_vs_amd import _lib

    def boom(rc, what):
        raise RuntimeError("option call failed")
    prev = _lib.current_amp()
    monkeypatch.setattr(_lib, "check", boom)
    try:
        with pytest.raises(RuntimeError):
            with _lib.train_amp(1 if prev != 1 else 2):
                pass
    finally:
        monkeypatch.undo()
        # the failure is simulated AFTER the library accepted the option: put the library's own setting back, or every later
        # training-tier call in this process (the GPU tests of the same session) would run its GEMMs on 16-bit products
        _lib.check(_lib.lib().axvs_set_option(b"train_amp", prev), "axvs_set_option")
    assert _lib.current_amp() == prev
    assert _lib._AMP_LOCK.acquire(blocking=False)       # free again (an RLock held by this thread would also succeed: check the count)
    _lib._AMP_LOCK.release()
    import threading
    got = []
    def other():
        ok = _lib._AMP_LOCK.acquire(timeout=2)
        got.append(ok)
        if ok:
            _lib._AMP_LOCK.release()
    t = threading.Thread(target=other)
    t.start(); t.join()
    assert got == [True], "another thread must be able to take the lock"


def test_in_place_levels_fall_back_when_the_strided_workspace_explodes():
    """advisor (round 4): a small level inside a long token buffer (B*T = 32 frames of 21504 tokens, a 32 x 32 level) would take
    ~680 MB per row-addressed temporary in place against 32 MB in the natural layout: can_run_in_place says no, the split / cat
    data flow runs; BASELINE config 3's stride is fine."""
    import axial_vs_amd as ax
    from axial_vs_amd import modules
    layer = ax.TemporalAxialTrajectoryAttentionLayer(256, 1024, n_heads=8).eval()
    pos_small = modules.tag_sine3d(torch.zeros(1, 4, 32, 32, 256), 10000.0, True, 6.283185307179586)
    assert layer.can_run_in_place(pos_small) and layer.can_run_in_place(pos_small, frame_stride_rows=64 * 64 + 32 * 32 + 16 * 16)
    pos_many = modules.tag_sine3d(torch.zeros(8, 4, 32, 32, 256), 10000.0, True, 6.283185307179586)
    assert not layer.can_run_in_place(pos_many, frame_stride_rows=21504)
    assert not layer.can_run_in_place(pos_many, frame_stride_rows=2 ** 22)      # row indices beyond 32 bits / 64


def _short_workspace_calls():
    """(entry point, its size query's value, call with `ws` workspace bytes) for every eval-tier *_fwd that takes workspace_bytes.
    Pointers are made up (distinct, 16-byte aligned, never dereferenced: the workspace check comes before any device work);
    arguments the host reads before that check (spatial_shapes, rates, the sine specification) are real host objects."""
    from axial_vs_amd import _lib
    L = _lib.lib()
    p = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(8)]
    B, T, H, W, C, h, F = 1, 2, 16, 12, 256, 8, 1024
    sine = ctypes.pointer(_lib.AxvsSinePos3D(10000.0, 1, 6.283, None))
    rates = (ctypes.c_int * 3)(1, 2, 3)
    shapes = (ctypes.c_int * 4)(8, 8, 4, 4)          # two levels, S = 80
    layers = (ctypes.c_void_p * 2)(0x90000, 0xa0000)
    N, S, Lq, nl, P = 2, 80, 80, 2, 4
    Q, Tc, V, K1, Cm, fpc = 16, 3, 2, 25, 256, 2
    stride = H * W + 40
    return [
        ("axvs_traj_attn_fwd", L.axvs_traj_attn_workspace_bytes(4, T, 16, C, h),
         lambda ws: L.axvs_traj_attn_fwd(p[0], p[0], p[0], p[1], None, p[2], 4, T, 16, C, h, 0, p[3], ws, None)),
        ("axvs_axial_layer_fwd", L.axvs_axial_layer_workspace_bytes_ex(B, T, H, W, C, h, F, 0, 0),
         lambda ws: L.axvs_axial_layer_fwd(p[0], p[1], p[2], p[3], B, T, H, W, C, h, F, 0, p[4], ws, None, None, None)),
        ("axvs_axial_layer_fwd[attention maps]", L.axvs_axial_layer_workspace_bytes_ex(B, T, H, W, C, h, F, 1, 0),
         lambda ws: L.axvs_axial_layer_fwd(p[0], p[1], p[2], p[3], B, T, H, W, C, h, F, 0, p[4], ws, p[5], p[6], None)),
        ("axvs_axial_layer_fwd_sine3d", L.axvs_axial_layer_workspace_bytes_ex(B, T, H, W, 128, h, F, 0, 1),
         lambda ws: L.axvs_axial_layer_fwd_sine3d(p[0], sine, p[2], p[3], B, T, H, W, 128, h, F, 0, p[4], ws, None, None, None)),
        ("axvs_axial_layer_fwd_sine3d_strided", L.axvs_axial_layer_workspace_bytes_strided(B, T, H, W, C, h, F, stride),
         lambda ws: L.axvs_axial_layer_fwd_sine3d_strided(p[0], sine, p[2], p[3], B, T, H, W, C, h, F, 0, stride, p[4], ws, None)),
        ("axvs_axial_pass_fwd", L.axvs_axial_layer_workspace_bytes_ex(B, T, H, W, C, h, F, 0, 0),
         lambda ws: L.axvs_axial_pass_fwd(p[0], p[1], p[2], p[3], 1, B, T, H, W, C, h, F, 0, p[4], ws, None)),
        ("axvs_traj_layer_fwd", L.axvs_traj_layer_workspace_bytes(B, T, H * W, C, h, F),
         lambda ws: L.axvs_traj_layer_fwd(p[0], p[1], p[2], p[3], B, T, H * W, C, h, F, 0, p[4], ws, None)),
        ("axvs_ffn_fwd", L.axvs_ffn_workspace_bytes(300, C, F),
         lambda ws: L.axvs_ffn_fwd(p[0], p[1], p[2], 300, C, h, F, 0, p[3], ws, None)),
        ("axvs_ffn_packed_fwd", L.axvs_ffn_workspace_bytes(300, C, F),
         lambda ws: L.axvs_ffn_packed_fwd(p[0], p[1], p[2], 300, C, F, 0, p[3], ws, None)),
        ("axvs_cc_layer_fwd", L.axvs_cc_layer_workspace_bytes(B, Q, Tc),
         lambda ws: L.axvs_cc_layer_fwd(p[0], p[1], p[2], B, Q, Tc, rates, 0, p[3], ws, None)),
        ("axvs_cc_heads_fwd", L.axvs_cc_heads_workspace_bytes(B, Q, Tc),
         lambda ws: L.axvs_cc_heads_fwd(p[0], p[1], p[2], p[3], p[4], B, Q, Tc, V, 8, 8, K1, 0, p[5], ws, None)),
        ("axvs_cc_module_fwd", L.axvs_cc_module_workspace_bytes(B, Q, Tc, nl),
         lambda ws: L.axvs_cc_module_fwd(p[0], p[1], p[2], p[3], p[4], layers, p[5], nl, B, Q, Tc, V, 8, 8, K1, rates, 0, p[6], ws, None)),
        ("axvs_tl_cc_module_fwd", L.axvs_tl_cc_module_workspace_bytes(B, Q, Tc, Cm, nl),
         lambda ws: L.axvs_tl_cc_module_fwd(p[0], p[1], p[2], p[3], p[4], layers, p[5], nl, B, Q, Tc, fpc, 8, 8, K1, Cm, rates, 0, p[6], ws, None)),
        ("axvs_tl_heads_fwd", L.axvs_tl_heads_workspace_bytes(B, Q, Tc, Cm),
         lambda ws: L.axvs_tl_heads_fwd(p[0], p[1], p[2], p[3], p[4], B, Q, Tc, fpc, 8, 8, K1, Cm, 0, p[5], ws, None)),
        ("axvs_msda_fwd", L.axvs_msda_workspace_bytes(N, Lq, S, C, h, 2, P),
         lambda ws: L.axvs_msda_fwd(p[0], p[1], 2, p[2], None, shapes, p[3], p[4], N, Lq, S, C, h, 2, P, 0, p[5], ws, None)),
        ("axvs_msda_sample_fwd", L.axvs_msda_workspace_bytes(N, Lq, S, C, h, 2, P),
         lambda ws: L.axvs_msda_sample_fwd(p[0], None, p[1], 2, p[2], None, shapes, p[3], p[4], N, Lq, S, C, h, 2, P, 0, p[5], ws, None)),
        ("axvs_msda_layer_fwd", L.axvs_msda_layer_workspace_bytes(N, S, C, h, 2, P, F),
         lambda ws: L.axvs_msda_layer_fwd(p[0], p[1], p[2], 2, None, shapes, p[3], p[4], N, S, C, h, 2, P, F, 0, p[5], ws, None)),
        ("axvs_conv1x1_gn_fwd", L.axvs_conv1x1_gn_workspace_bytes(N, 99, 256, 32),
         lambda ws: L.axvs_conv1x1_gn_fwd(p[0], 0, 512 * 99, 99, p[1], 1, 99 * 256, 256, p[2], N, 99, 512, 256, 32, 1e-5, 0, p[3], ws, None)),
        ("axvs_fpn_level_fwd", L.axvs_fpn_level_workspace_bytes(N, 10, 14, 512, 256, 32),
         lambda ws: L.axvs_fpn_level_fwd(p[0], p[1], 5 * 7 * 256, 256, 5, 7, p[2], None, p[3], N, 10, 14, 512, 256, 0, 32, 1e-5, 0, p[4], ws, None)),
    ]


def test_every_forward_refuses_a_workspace_one_byte_short():
    """The workspace contract of include/axvs.h: a *_fwd entry point called with fewer bytes than its size query asks for returns
    AXVS_ERR_WORKSPACE (-2) before any device work, and the error text holds both sizes.  (Every eval-tier entry point makes its
    workspace check before it touches the device, so none is left out.)"""
    from axial_vs_amd import _lib
    L = _lib.lib()
    calls = _short_workspace_calls()
    names = {n.split("[")[0] for n, _, _ in calls}
    eval_fwd = {n for n, (_, args) in _lib.SIGNATURES.items() if n.endswith("_fwd") or "_fwd_" in n
                if "_train_" not in n and ctypes.c_size_t in args}
    assert names == eval_fwd, sorted(names ^ eval_fwd)
    for name, need, call in calls:
        assert need > 0, name
        rc = call(need - 1)
        err = L.axvs_last_error().decode()
        assert rc == -2, (name, rc, err)
        assert str(need - 1) in err and str(need) in err and "workspace too small" in err, (name, err)


def _short_training_calls():
    """(entry point, saved bytes, scratch bytes, call with (saved_bytes, scratch_bytes)) for every *_train_fwd / *_train_bwd, at the
    smallest shapes each family takes.  Pointers are made up as in _short_workspace_calls (the size check comes before any device
    work); what the host reads before that check (configurations, spatial_shapes, the fields of the parameter structs) is real."""
    from axial_vs_amd import _lib
    L = _lib.lib()
    p = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(10)]

    def full(cls, n=1):      # n structs of `cls`, every field a made-up non-null pointer
        k = ctypes.sizeof(cls) // ctypes.sizeof(ctypes.c_void_p)
        one = [_lib.fill(cls, [ctypes.c_void_p(0x100000 + 64 * (j * k + i)) for i in range(k)]) for j in range(n)]
        return (cls * n)(*one)
    B, T, H, W, C, h, F = 1, 2, 4, 4, 64, 8, 64
    ax, tj, md = full(_lib.AxvsAxialLayerParams), full(_lib.AxvsTrajLayerParams), full(_lib.AxvsMsdaLayerParams)
    shapes = (ctypes.c_int * 4)(4, 4, 2, 2)          # two levels, S = 20
    N, S, nlv, P = 1, 20, 2, 4
    cc = _lib.AxvsCCTrainCfg(B=1, Q=8, Tc=2, V=1, H=4, W=4, K1=3, num_layers=2, rates=(ctypes.c_int * 3)(1, 2, 3))
    chain = _lib.AxvsCCTrainCfg(B=1, Q=8, Tc=2, num_layers=2, rates=(ctypes.c_int * 3)(1, 2, 3), chain_only=1)
    ccl, cch, cchg = full(_lib.AxvsCCLayerParams, 2), full(_lib.AxvsCCHeadParams), full(_lib.AxvsCCHeadGrads)
    tl = _lib.AxvsTLHeadTrainCfg(B=1, Q=4, Tc=2, frames_per_clip=1, h=4, w=4, K1=3, Cm=128, num_layers=1)
    tlp, tlg = full(_lib.AxvsTLHeadParams), full(_lib.AxvsTLHeadGrads)
    gn = full(_lib.AxvsConvGnParams)
    HW, Cin, Cout, G = 16, 8, 8, 2
    cg = (HW * Cin, HW)                              # NCHW: batch stride, row stride
    co = (HW * Cout, HW)
    conv_saved = L.axvs_conv1x1_gn_train_saved_bytes(N, HW, Cin, Cout, G, 0, *cg)
    return [
        ("axvs_axial_layer_train_fwd", L.axvs_axial_layer_train_saved_bytes(B, T, H, W, C, h, F), L.axvs_axial_layer_train_scratch_bytes(B, T, H, W, C, h, F, 0),
         lambda sv, sc: L.axvs_axial_layer_train_fwd(p[0], p[1], p[2], ax, B, T, H, W, C, h, F, 0.1, 0.1, 7, p[3], sv, p[4], sc, None)),
        ("axvs_axial_layer_train_bwd", L.axvs_axial_layer_train_saved_bytes(B, T, H, W, C, h, F), L.axvs_axial_layer_train_scratch_bytes(B, T, H, W, C, h, F, 1),
         lambda sv, sc: L.axvs_axial_layer_train_bwd(p[0], p[1], p[2], ax, ax, p[3], p[4], B, T, H, W, C, h, F, 0.1, 0.1, 7, 0, p[5], sv, p[6], sc, None)),
        ("axvs_traj_layer_train_fwd", L.axvs_traj_layer_train_saved_bytes(B, T, H * W, C, h, F), L.axvs_traj_layer_train_scratch_bytes(B, T, H * W, C, h, F, 0),
         lambda sv, sc: L.axvs_traj_layer_train_fwd(p[0], p[1], p[2], tj, B, T, H * W, C, h, F, 0.1, 0.1, 7, p[3], sv, p[4], sc, None)),
        ("axvs_traj_layer_train_bwd", L.axvs_traj_layer_train_saved_bytes(B, T, H * W, C, h, F), L.axvs_traj_layer_train_scratch_bytes(B, T, H * W, C, h, F, 1),
         lambda sv, sc: L.axvs_traj_layer_train_bwd(p[0], p[1], p[2], tj, tj, p[3], p[4], B, T, H * W, C, h, F, 0.1, 0.1, 7, 1, p[5], sv, p[6], sc, None)),
        ("axvs_msda_layer_train_fwd", L.axvs_msda_layer_train_saved_bytes(N, S, C, h, nlv, P, F), L.axvs_msda_layer_train_scratch_bytes(N, S, C, h, nlv, P, F, 0),
         lambda sv, sc: L.axvs_msda_layer_train_fwd(p[0], p[1], p[2], 2, None, shapes, p[3], md, N, S, C, h, nlv, P, F, 0.1, 0.1, 7, p[4], sv, p[5], sc, None)),
        ("axvs_msda_layer_train_bwd", L.axvs_msda_layer_train_saved_bytes(N, S, C, h, nlv, P, F), L.axvs_msda_layer_train_scratch_bytes(N, S, C, h, nlv, P, F, 1),
         lambda sv, sc: L.axvs_msda_layer_train_bwd(p[0], p[1], p[2], p[3], 2, None, shapes, md, md, p[4], p[5], N, S, C, h, nlv, P, F, 0.1, 0.1, 7, 0,
                                                    p[6], sv, p[7], sc, None)),
        ("axvs_cc_module_train_fwd", L.axvs_cc_module_train_saved_bytes(cc), L.axvs_cc_module_train_scratch_bytes(cc, 0),
         lambda sv, sc: L.axvs_cc_module_train_fwd(p[0], p[1], p[2], p[3], p[4], ccl, cch, cc, p[5], sv, p[6], sc, None)),
        ("axvs_cc_module_train_bwd", L.axvs_cc_module_train_saved_bytes(cc), L.axvs_cc_module_train_scratch_bytes(cc, 1),
         lambda sv, sc: L.axvs_cc_module_train_bwd(p[0], p[1], p[2], p[3], ccl, cch, ccl, cchg, p[4], cc, p[5], sv, p[6], sc, None)),
        ("axvs_cc_layers_train_fwd", L.axvs_cc_module_train_saved_bytes(chain), L.axvs_cc_module_train_scratch_bytes(chain, 0),
         lambda sv, sc: L.axvs_cc_layers_train_fwd(p[0], p[1], ccl, chain, p[2], sv, p[3], sc, None)),
        ("axvs_cc_layers_train_bwd", L.axvs_cc_module_train_saved_bytes(chain), L.axvs_cc_module_train_scratch_bytes(chain, 1),
         lambda sv, sc: L.axvs_cc_layers_train_bwd(p[0], p[1], ccl, ccl, p[2], chain, p[3], sv, p[4], sc, None)),
        ("axvs_tl_heads_train_fwd", L.axvs_tl_heads_train_saved_bytes(tl), L.axvs_tl_heads_train_scratch_bytes(tl, 0),
         lambda sv, sc: L.axvs_tl_heads_train_fwd(p[0], p[1], p[2], p[3], tlp, tl, p[4], sv, p[5], sc, None)),
        ("axvs_tl_heads_train_bwd", L.axvs_tl_heads_train_saved_bytes(tl), L.axvs_tl_heads_train_scratch_bytes(tl, 1),
         lambda sv, sc: L.axvs_tl_heads_train_bwd(p[0], p[1], p[2], p[3], tlp, tlg, p[4], p[5], tl, p[6], sv, p[7], sc, None)),
        ("axvs_conv1x1_gn_train_fwd", conv_saved, L.axvs_conv1x1_gn_train_scratch_bytes(N, HW, Cin, Cout, G, 0),
         lambda sv, sc: L.axvs_conv1x1_gn_train_fwd(p[0], 0, *cg, p[1], 0, *co, gn, N, HW, Cin, Cout, G, 1e-5, p[2], sv, p[3], sc, None)),
        ("axvs_conv1x1_gn_train_bwd", conv_saved, L.axvs_conv1x1_gn_train_scratch_bytes(N, HW, Cin, Cout, G, 1),
         lambda sv, sc: L.axvs_conv1x1_gn_train_bwd(p[0], 0, *co, p[1], 0, *cg, gn, gn, p[2], N, HW, Cin, Cout, G, p[3], sv, p[4], sc, None)),
    ]


def test_every_training_entry_point_refuses_buffers_one_byte_short():
    """The buffer contract of the training tier (include/axvs.h): a *_train_fwd / *_train_bwd called with one byte less than either of
    its size queries asks for -- saved_bytes, then scratch_bytes -- returns AXVS_ERR_WORKSPACE (-2) before any device work, and the
    error text holds the short size and the needed one.  Every training entry point is covered: the names come from SIGNATURES."""
    from axial_vs_amd import _lib
    L = _lib.lib()
    calls = _short_training_calls()
    train = {n for n in _lib.SIGNATURES if n.endswith("_train_fwd") or n.endswith("_train_bwd")}
    assert {n for n, _, _, _ in calls} == train, sorted({n for n, _, _, _ in calls} ^ train)
    for name, saved, scratch, call in calls:
        assert saved > 0 and scratch > 0, (name, saved, scratch)
        for sv, sc, short, need in ((saved - 1, scratch, saved - 1, saved), (saved, scratch - 1, scratch - 1, scratch)):
            rc = call(sv, sc)
            err = L.axvs_last_error().decode()
            assert rc == -2, (name, rc, err)
            assert f"{short} < {need}" in err and "training buffers too small" in err, (name, err)


def _negative_workspace_calls():
    """(entry point, call with `ws` workspace bytes) for one *_fwd of each unit whose ABI takes `long long workspace_bytes`, at the
    smallest configuration the unit accepts.  Pointers are made up as in _short_workspace_calls."""
    from axial_vs_amd import _lib
    L = _lib.lib()
    by = ctypes.byref
    p = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(12)]
    i3, i4 = ctypes.c_int * 3, ctypes.c_int * 4
    arr = lambda n: (ctypes.c_void_p * n)(*[0x100000 * (i + 1) for i in range(n)])
    one = (ctypes.c_int * 1)(1)
    m2f = _lib.AxvsM2fCfg(N=1, Q=1, T=1, C=256, heads=8, ffn=2048, num_layers=1, num_levels=3, K1=1, h=1, w=1, lh=i3(1, 1, 1), lw=i3(1, 1, 1),
                          return_predictions=0, pos_normalize=1, pos_temperature=10000.0, pos_scale=6.283185307179586)
    kmax = _lib.AxvsKmaxCfg(B=1, T=1, L=1, K1=1, num_layers=1, in_channels=i3(16, 16, 16), h=i3(1, 1, 1), w=i3(1, 1, 1), pan_channels=256, H=1, W=1,
                            heads=8, base_filters=128, want_masks=0, want_pixel_feature=0)
    kpix = _lib.AxvsKpixCfg(N=1, in_channels=i4(16, 16, 16, 16), h=i4(1, 1, 1, 1), w=i4(1, 1, 1, 1), base=i4(32, 32, 32, 32), blocks=i4(1, 1, 1, 1),
                            axial=i4(0, 0, 0, 0), heads=8)
    cnx = _lib.AxvsCnxCfg(N=1, H=1, W=1, dims=i4(16, 16, 16, 16), depths=i4(1, 1, 1, 1), h=i4(1, 1, 1, 1), w=i4(1, 1, 1, 1), v2=0)
    vis = _lib.AxvsVisCfg(Q=1, K1=2, T=1, num_frames=1, h=1, w=1, image_h=1, image_w=1, crop_h=1, crop_w=1, H=1, W=1, num_things=0, k_cand=1, k_out=1,
                          mask_bits=0)
    pan = _lib.AxvsPanopticCfg(N=1, K1=2, T=1, h=1, w=1, image_h=1, image_w=1, two_stage=0, crop_h=0, crop_w=0, H=1, W=1, align_corners=0,
                               label_divisor=0, pixel_confidence_threshold=0.4, overlap_threshold=0.8, class_threshold_thing=0.7,
                               class_threshold_stuff=0.5, reorder_class_weight=1.0, reorder_mask_weight=1.0)
    tl = _lib.AxvsTLLossCfg(L=1, B=1, Q=1, K1=2, T=1, h=1, w=1, Hg=1, Wg=1, num_points=1, num_cand=0, num_kept=0, target_dtype=_lib.AXVS_U8,
                            cost_cls=2, cost_mask=5, cost_dice=5, loss_cls=2, loss_mask=5, loss_dice=5, dice_eps=1)
    return [
        ("axvs_m2f_decoder_fwd", lambda ws: L.axvs_m2f_decoder_fwd(by(m2f), p[0], p[1], arr(3), p[2], None, None, None, None, p[3], ws, None)),
        ("axvs_kmax_decoder_fwd", lambda ws: L.axvs_kmax_decoder_fwd(by(kmax), p[0], arr(3), None, p[1], None, p[2], None, p[3], None, p[4], ws, None)),
        ("axvs_kmax_pix_decoder_fwd", lambda ws: L.axvs_kmax_pix_decoder_fwd(by(kpix), p[0], arr(4), arr(4), p[1], ws, None)),
        ("axvs_cnx_fwd", lambda ws: L.axvs_cnx_fwd(by(cnx), p[0], p[1], arr(5), p[2], ws, None)),
        ("axvs_video_instance_fwd", lambda ws: L.axvs_video_instance_fwd(by(vis), p[0], p[1], _lib.AXVS_F32, p[2], p[3], p[4], p[5], ws, None)),
        ("axvs_video_panoptic_fwd",
         lambda ws: L.axvs_video_panoptic_fwd(by(pan), p[0], p[1], _lib.AXVS_F32, p[2], p[3], p[4], p[5], p[6], p[7], ws, None)),
        ("axvs_set_criterion_fwd",
         lambda ws: L.axvs_set_criterion_fwd(arr(1), arr(1), p[0], _lib.AXVS_U8, p[1], one, p[2], p[3], p[4], p[5], 1, 1, 1, 1, 2, 1, 1, 1, p[6], p[7], p[8],
                                             ws, None)),
        ("axvs_pixel_insdis_fwd",
         lambda ws: L.axvs_pixel_insdis_fwd(arr(1), p[0], _lib.AXVS_U8, one, p[1], 1, 1, 1, 1, 1, 4, 1, p[2], 1, 1, p[3], p[4], p[5], ws, None)),
        ("axvs_tl_loss_fwd",
         lambda ws: L.axvs_tl_loss_fwd(by(tl), arr(1), arr(1), p[0], p[1], one, p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], None, None, p[10], p[11],
                                       ws, None)),
    ]


def test_every_signed_workspace_size_refuses_a_negative_one():
    """The units whose ABI takes `long long workspace_bytes` (the query decoders, the pixel decoder, the backbone, the two post-processing
    units and the three loss units) share one workspace check: a negative size is too small, whatever it would be as an unsigned number.
    AXVS_ERR_WORKSPACE (-2) with the size in the text, before any device work.  One entry point per unit: the names come from
    SIGNATURES, so a new unit with a signed size has to add its case."""
    from axial_vs_amd import _lib
    L = _lib.lib()
    calls = _negative_workspace_calls()
    signed = {n for n, (_, args) in _lib.SIGNATURES.items() if n.endswith("_fwd") and "_train_" not in n and args[-2:] == [ctypes.c_longlong, _lib._fp]}
    units = ("axvs_m2f_", "axvs_kmax_pix_", "axvs_kmax_", "axvs_cnx_", "axvs_video_instance_", "axvs_video_panoptic_", "axvs_set_criterion_",
             "axvs_pixel_", "axvs_tl_loss_")                     # (the first prefix that fits: axvs_kmax_pix_ in front of axvs_kmax_)
    unit_of = lambda n: next((u for u in units if n.startswith(u)), n)
    assert {n for n, _ in calls} <= signed
    assert sorted(unit_of(n) for n, _ in calls) == sorted({unit_of(n) for n in signed}) == sorted(units)
    for name, call in calls:
        rc = call(-1)
        err = L.axvs_last_error().decode()
        assert rc == -2, (name, rc, err)
        assert "workspace too small" in err and "-1" in err, (name, err)


def _target_unit_calls():
    """unit -> (its name for the query count, call(L, B, Q, m, tdt, layers, M_max)): one forward entry point of each training-target unit
    at L layers x B videos with Q queries, K + 1 = 3 logits and 130 pixels (TL: T = 2, h = w = 8, 32 points).  `layers` are the per-layer
    prediction pointers (None: NULL); every other pointer is made up as in _short_workspace_calls."""
    from axial_vs_amd import _lib
    lib = _lib.lib()
    p = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(12)]
    arr = lambda layers: (ctypes.c_void_p * len(layers))(*layers)
    ints = lambda m: (ctypes.c_int * len(m))(*m)
    big = 1 << 40

    def matcher(L, B, Q, m, tdt, layers, M_max):
        return lib.axvs_video_matcher(arr(layers), _lib.AXVS_F32, arr(layers), p[0], tdt, p[1], ints(m), L, B, Q, 3, 130, M_max, 1, p[2], p[3], p[4], p[5],
                                      p[6], p[7], big, None)

    def criterion(L, B, Q, m, tdt, layers, M_max):
        return lib.axvs_set_criterion_fwd(arr(layers), arr(layers), p[0], tdt, p[1], ints(m), p[2], p[3], p[4], p[5], 1, L, B, Q, 3, 130, 1, 0, p[6], p[7],
                                          p[8], big, None)

    def insdis(L, B, Q, m, tdt, layers, M_max):
        return lib.axvs_pixel_insdis_fwd(arr(layers), p[0], tdt, ints(m), p[1], 1, 0, L, B, Q, 4, 130, p[2], 16, 16, p[3], p[4], p[5], big, None)

    def tl(L, B, Q, m, tdt, layers, M_max):
        cfg = _lib.AxvsTLLossCfg(L=L, B=B, Q=Q, K1=3, T=2, h=8, w=8, Hg=8, Wg=8, num_points=32, num_cand=0, num_kept=0, target_dtype=tdt,
                                 cost_cls=2, cost_mask=5, cost_dice=5, loss_cls=2, loss_mask=5, loss_dice=5, dice_eps=1)
        return lib.axvs_tl_loss_fwd(ctypes.byref(cfg), arr(layers), arr(layers), p[0], p[1], ints(m), p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], None,
                                    None, p[10], p[11], big, None)

    return {"matcher": ("Q", matcher), "criterion": ("N", criterion), "pixel": ("N", insdis), "tl": ("Q", tl)}


@pytest.mark.parametrize("unit", ["matcher", "criterion", "pixel", "tl"])
def test_target_units_refuse_each_out_of_bounds_argument_by_name(unit):
    """The matcher, the set criterion, the sampled pixel losses and Tube-Link's loss take the same kind of input (L layers x B videos,
    per-layer pointers, m_per_video, u8 / fp32 targets) and share its checks: with ONE argument out of bounds the forward returns
    AXVS_ERR_ARG before any device work, and the text names the offending value and its bound."""
    from axial_vs_amd import _lib
    lib = _lib.lib()
    q, call = _target_unit_calls()[unit]
    mb = lambda bound: f"0..M_max={bound}" if unit == "matcher" else "0..512"      # the matcher's bound on an entry is the caller's M_max
    cases = [(dict(L=0), ["L=0", "1..16"]), (dict(L=17), ["L=17", "1..16"]), (dict(B=65), ["B=65", "1..64"]), (dict(Q=513), [f"{q}=513", "1..512"]),
             (dict(m=[-1, 3]), ["m_per_video[0]=-1", mb(3)]), (dict(m=[3, 513], M_max=512), ["m_per_video[1]=513", mb(512)]),
             (dict(tdt=_lib.AXVS_F16), ["target dtype 0", "AXVS_F32 / AXVS_U8"]), (dict(null_layer=1), ["null pointer (layer 1)"])]
    if unit == "matcher":
        cases.append((dict(M_max=4), ["M_max=4", "largest entry of m_per_video (3)"]))
    for kw, words in cases:
        L, B = kw.get("L", 2), kw.get("B", 2)
        m = kw.get("m", [3] + [0] * (B - 1))
        layers = [0x100000 * (i + 1) for i in range(max(L, 1))]
        if "null_layer" in kw:
            layers[kw["null_layer"]] = None
        rc = call(L, B, kw.get("Q", 8), m, kw.get("tdt", _lib.AXVS_U8), layers, kw.get("M_max", max(m)))
        err = lib.axvs_last_error().decode()
        assert rc == -1, (unit, kw, rc, err)
        assert all(w in err for w in words), (unit, kw, err)


def _inference_unit_calls():
    """family -> [(what is wrong, call(dtype), words of the message)]: entry points of the three inference units (axial, cross-clip, pixel
    decoder), each called with ONE wrong argument.  Pointers are made up as in _short_workspace_calls; what the host reads before the
    failing check (spatial_shapes, rates, the parameter struct's address) is real."""
    from axial_vs_amd import _lib
    L = _lib.lib()
    p = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(8)]
    B, T, H, W, C, h, F = 1, 2, 16, 12, 256, 8, 1024
    Q, Tc, K1, fpc = 16, 3, 25, 2
    N, S, Lq, P = 2, 80, 80, 4
    rates = (ctypes.c_int * 3)(1, 2, 3)
    shapes = (ctypes.c_int * 4)(8, 8, 4, 4)          # two levels, S = 80
    tlp = ctypes.byref(_lib.AxvsTLHeadParams())
    big = 1 << 40

    def axial_pass(dtype, pass_=1, src=p[0]):
        return L.axvs_axial_pass_fwd(src, p[1], p[2], p[3], pass_, B, T, H, W, C, h, F, dtype, p[4], big, None)

    def cc_layer(dtype, ws=big, out=p[1]):
        return L.axvs_cc_layer_fwd(p[0], out, p[2], B, Q, Tc, rates, dtype, p[3], ws, None)

    def msda(dtype, ref_dim=2):
        return L.axvs_msda_fwd(p[0], p[1], ref_dim, p[2], None, shapes, p[3], p[4], N, Lq, S, C, h, 2, P, dtype, p[5], big, None)

    def fpn(dtype, groups=32):
        return L.axvs_fpn_level_fwd(p[0], p[1], 5 * 7 * 256, 256, 5, 7, p[2], None, p[3], N, 10, 14, 512, 256, 0, groups, 1e-5, dtype, p[4], big, None)

    cc_need = L.axvs_cc_layer_workspace_bytes(B, Q, Tc)
    return {
        "axial": (axial_pass, [
            ("pass = 2", lambda dt: axial_pass(dt, pass_=2), -1, ["pass must be 0 (height) or 1 (width + FFN)"]),
            ("null src", lambda dt: axial_pass(dt, src=None), -1, ["null pointer"])]),
        "cross-clip": (cc_layer, [
            ("Cm = 64", lambda dt: L.axvs_tl_heads_pack(tlp, p[0], K1, 64, dt, None), -1, ["mask feature channels must be 128 or 256 (got 64)"]),
            ("null out", lambda dt: cc_layer(dt, out=None), -1, ["null pointer"]),
            ("workspace one byte short", lambda dt: cc_layer(dt, ws=cc_need - 1), -2, ["workspace too small", f"{cc_need - 1} < {cc_need}"])]),
        "pixel decoder": (msda, [
            ("ref_dim = 3", lambda dt: msda(dt, ref_dim=3), -1, ["Last dim of reference_points must be 2 or 4, but get 3 instead."]),
            ("groups = 7", lambda dt: fpn(dt, groups=7), -1, ["groups=7 must divide C=256"])]),
    }


@pytest.mark.parametrize("family", ["axial", "cross-clip", "pixel decoder"])
def test_inference_units_refuse_each_wrong_argument_by_name(family):
    """The axial, cross-clip and pixel-decoder entry points live in three translation units that share their argument checks (dtype,
    configuration, workspace): a call with one wrong argument returns its error code before any device work and axvs_last_error() names
    what was wrong -- and a library built without the bf16 operand tier refuses AXVS_BF16 in every one of the three."""
    from axial_vs_amd import _lib
    L = _lib.lib()
    entry, cases = _inference_unit_calls()[family]
    for what, call, code, words in cases:
        rc = call(_lib.AXVS_F16)
        err = L.axvs_last_error().decode()
        assert rc == code, (family, what, rc, err)
        assert all(w in err for w in words), (family, what, err)
    if not L.axvs_has_bf16():
        rc = entry(_lib.AXVS_BF16)
        err = L.axvs_last_error().decode()
        assert rc == -1 and "the bf16 operand tier is not built into this library" in err, (family, rc, err)
    rc = entry(7)
    assert rc == -1 and "unknown dtype 7" in L.axvs_last_error().decode(), (family, rc)
