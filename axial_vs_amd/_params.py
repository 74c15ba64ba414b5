"""The order of every C parameter struct of include/axvs.h (mirrored in _lib.py), stated once: one function per struct that takes
the owning module(s) and returns the parameter tensors in the struct's declaration order -- what `_lib.fill` consumes.

The functions return the `nn.Parameter` objects themselves (no detach, no cast).  The training tier hands them to autograd as inputs
and fills parameter and gradient structs from their pointers; the eval tier casts them once and fills the same structs to pack
(modules._pack_weights).
"""
from __future__ import annotations

from typing import List, Optional, Sequence

from torch import Tensor

from . import _lib


def _wb(*mods) -> List[Tensor]:
    return [t for m in mods for t in (m.weight, m.bias)]


def _tail(layer) -> List[Tensor]:
    return _wb(layer.norm1, layer.linear1, layer.linear2, layer.norm2)


def traj_params(attn) -> List[Tensor]:
    """AxvsTrajParams of a within-clip TrajectoryAttention (separate q / k / v projections)."""
    return _wb(attn.q, attn.k, attn.v, attn.proj_q, attn.proj_kv, attn.proj)


def axial_layer_params(layer) -> List[Tensor]:
    """AxvsAxialLayerParams of a TemporalAxialTrajectoryAttentionLayer."""
    return traj_params(layer.height_attn) + traj_params(layer.width_attn) + _tail(layer)


def traj_layer_params(layer) -> List[Tensor]:
    """AxvsTrajLayerParams of a TemporalTrajectoryAttentionLayer."""
    return traj_params(layer.temporal_attn) + _tail(layer)


def msda_params(attn) -> List[Tensor]:
    """AxvsMsdaParams of an MSDeformAttn or of Tube-Link's MultiScaleDeformableAxialTrajectoryAttention (same member names)."""
    return _wb(attn.value_proj, attn.sampling_offsets, attn.attention_weights, attn.output_proj)


def msda_layer_params(layer) -> List[Tensor]:
    """AxvsMsdaLayerParams of an MSDeformAttnTransformerEncoderLayer."""
    return msda_params(layer.self_attn) + _tail(layer)


def conv_gn_params(conv, gn) -> List[Tensor]:
    """AxvsConvGnParams of a 1x1 convolution and its GroupNorm (conv.weight is [Cout, Cin, 1, 1]: the bytes of [Cout, Cin])."""
    return _wb(conv, gn)


def ffn_params(layer) -> List[Tensor]:
    """AxvsFfnParams of an encoder layer of Tube-Link's pixel decoder: norms[0] -> FFN (two Linear layers) -> norms[1]."""
    fcs = layer.ffns[0].layers
    return _wb(layer.norms[0], fcs[0][0], fcs[1], layer.norms[1])


def fpn_level_params(lateral, output, mask_feature=None) -> List[Optional[Tensor]]:
    """AxvsFpnLevelParams of one FPN level (convolutions without bias); a level without the mask head has None in the last two slots."""
    return [lateral.conv.weight, lateral.gn.weight, lateral.gn.bias, output.conv.weight, output.gn.weight, output.gn.bias,
            None if mask_feature is None else mask_feature.weight, None if mask_feature is None else mask_feature.bias]


# ---- cross-clip modules ---------------------------------------------------------------------------------------------------------------
CC_PER_LAYER = 21      # tensors per cross-clip layer: the fused qkv counts once (AxvsCCLayerParams has 25 pointer slots)


def cc_layer_params(mod, i: int) -> List[Tensor]:
    """Layer `i` of a cross-clip module (trajectory layer, ASPP, LayerNorm) in AxvsCCLayerParams order, with two differences that
    `cc_layer_struct` undoes: the fused `qkv` projection stands for the q / k / v slots, and the ASPP convolutions come as
    (weight, bias) pairs."""
    lay, asp, cn = mod.transformer_trajectory_self_attention_layers[i], mod.conv_short_aggregate_layers[i], mod.conv_norms[i]
    at, pj = lay.self_attn, asp._proj_conv_bn_act
    return (_wb(at.qkv, at.proj_q, at.proj_kv, at.proj, lay.norm, asp._aspp_conv0, asp._aspp_conv1, asp._aspp_conv2)
            + [pj.conv.weight, pj.norm.weight, pj.norm.bias, cn.weight, cn.bias])


def cc_chain_params(mod, num_layers: int) -> List[Tensor]:
    return [t for i in range(num_layers) for t in cc_layer_params(mod, i)]


def cc_layer_struct(ptrs: Sequence[int], Cc: int = 256) -> _lib.AxvsCCLayerParams:
    """AxvsCCLayerParams (or AxvsCCLayerGrads: same layout) from the pointers of one layer's `cc_layer_params`: q / k / v are the three
    row blocks of the fused fp32 [3 Cc, Cc] weight and [3 Cc] bias."""
    if len(ptrs) != CC_PER_LAYER:
        raise ValueError(f"AxvsCCLayerParams takes {CC_PER_LAYER} pointers (fused qkv), got {len(ptrs)}")
    w, b = ptrs[0], ptrs[1]
    return _lib.fill(_lib.AxvsCCLayerParams, [w, b, w + 4 * Cc * Cc, b + 4 * Cc, w + 8 * Cc * Cc, b + 8 * Cc, *ptrs[2:10],
                                              *ptrs[10:16:2], *ptrs[11:16:2], *ptrs[16:]])


def cc_bn_modules(mod) -> list:
    """The four BatchNorm sites of a CrossClipTrackingModule's heads, in AxvsCCHeadParams order."""
    return [mod._class_embedding_projection.norm, mod._mask_embedding_projection.norm, mod._predictor._transformer_mask_head.norm,
            mod._predictor._pixel_space_mask_batch_norm]


def cc_head_params(mod) -> List[Tensor]:
    """The trainable tensors of a CrossClipTrackingModule's heads in AxvsCCHeadGrads order: AxvsCCHeadParams without the running
    statistics, which `cc_head_with_running` adds."""
    pr = mod._predictor
    bn = cc_bn_modules(mod)
    return ([mod._class_embedding_projection.conv.weight] + _wb(bn[0]) + [mod._mask_embedding_projection.conv.weight] + _wb(bn[1])
            + [pr._transformer_mask_head.conv.weight] + _wb(bn[2])
            + _wb(pr._transformer_class_head.conv, pr._transformer_class_activation_head.conv, bn[3]))


def cc_head_with_running(ps: Sequence, running: Sequence) -> list:
    """AxvsCCHeadParams order from `cc_head_params` order (tensors or pointers) and the (mean, var) pair of each BatchNorm site: every
    AxvsBN is (w, b, mean, var)."""
    ps = list(ps)
    return ps[0:3] + list(running[0]) + ps[3:6] + list(running[1]) + ps[6:9] + list(running[2]) + ps[9:15] + list(running[3])


def cc_module_params(mod) -> List[Tensor]:
    """Every trainable tensor of a CrossClipTrackingModule: the layer chain, then the heads."""
    return cc_chain_params(mod, mod.num_layers) + cc_head_params(mod)


def m2f_layer_params(layer) -> List[Tensor]:
    """AxvsM2fLayerParams of one DetrTransformerDecoderLayer of the per-clip query decoder: cross-attention, norm, self-attention, norm,
    FFN, norm."""
    ca, sa, fcs = layer.attentions[0].attn, layer.attentions[1].attn, layer.ffns[0].layers
    return ([ca.in_proj_weight, ca.in_proj_bias] + _wb(ca.out_proj, layer.norms[0]) + [sa.in_proj_weight, sa.in_proj_bias]
            + _wb(sa.out_proj, layer.norms[1], fcs[0][0], fcs[1], layer.norms[2]))


def m2f_head_params(mod) -> List[Tensor]:
    """AxvsM2fHeadParams of a TubeLinkClipDecoder: post_norm, the three embeddings, the mask_embed weights, then their biases, cls_embed."""
    me = mod.mask_embed
    return (_wb(mod.transformer_decoder.post_norm) + [mod.query_embed.weight, mod.query_feat.weight, mod.level_embed.weight,
                                                      me[0].weight, me[2].weight, me[4].weight, me[0].bias, me[2].bias, me[4].bias]
            + _wb(mod.cls_embed))


def tl_head_params(mod) -> List[Tensor]:
    """AxvsTLHeadParams of a TubeLinkCrossClipHead: post_norm, activation_proj, cls_embed, the three mask_embed weights, then their
    three biases."""
    me = mod.mask_embed
    return (_wb(mod.transformer_decoder.post_norm, mod.activation_proj, mod.cls_embed)
            + [me[0].weight, me[2].weight, me[4].weight, me[0].bias, me[2].bias, me[4].bias])
