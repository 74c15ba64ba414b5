"""The order of every C parameter struct of include/axvs.h (mirrored in _lib.py), stated once: one function per struct that takes
the owning module(s) and returns the parameter tensors in the struct's declaration order -- what `_lib.fill` consumes.

The functions return the `nn.Parameter` objects themselves (no detach, no cast).  The training tier hands them to autograd as inputs
and fills parameter and gradient structs from their pointers; the eval tier casts them once and fills the same structs to pack
(modules._pack_weights).
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import torch
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


# ---- Video-kMaX's k-means query decoder -------------------------------------------------------------------------------------------------
# AxvsKmaxLayerParams / AxvsKmaxHeadParams hold FOLDED tensors, so these functions return new float64 tensors, not the parameters: every
# BatchNorm is the affine map a x + c on its running statistics (eps 1e-3), folded into the convolution in front of it where there is
# one.  They read a mapping of the reference's own state-dict names (a module's parameters and buffers, or a checkpoint's tensors).
KMAX_BN_EPS = 1e-3


def kmax_predictor_shapes(K1: int) -> List[tuple]:
    """(slot, shape) of AxvsKmaxPredictorParams, in order"""
    return [("dw_w", (25, 256)), ("dw_b", (256,)), ("ph1_w", (256, 256)), ("ph1_b", (256,)), ("ph2_w", (128, 256)), ("ph2_b", (128,)),
            ("mh_w", (128, 256)), ("mh_b", (128,)), ("cls_w", (K1, 256)), ("cls_b", (K1,)), ("mask_ab", (4,))]


def kmax_layer_shapes(cin: int, K1: int) -> List[tuple]:
    """(slot, shape) of AxvsKmaxLayerParams, in order (_lib.KMAX_LAYER_FIELDS)"""
    return ([("pix1_w", (256, cin)), ("pix1_b", (256,)), ("q1_w", (256, 256)), ("q1_b", (256,))]
            + [("pred." + n, s) for n, s in kmax_predictor_shapes(K1)]
            + [("kv_w", (256, 260)), ("kv_b", (256,)), ("k3_w", (256, 256)), ("k3_b", (256,)), ("qkv_w", (512, 256)), ("qkv_b", (512,)),
               ("sim_ab", (16,)), ("rv_ab", (512,)), ("a3_w", (256, 256)), ("a3_b", (256,)), ("f1_w", (2048, 256)), ("f1_b", (2048,)),
               ("f2_w", (256, 2048)), ("f2_b", (256,))])


def kmax_head_shapes(L: int, K1: int) -> List[tuple]:
    """(slot, shape) of AxvsKmaxHeadParams, in order (_lib.KMAX_HEAD_FIELDS)"""
    return ([("centers", (L, 256)), ("cep_w", (256, 256)), ("cep_b", (256,)), ("mep_w", (256, 256)), ("mep_b", (256,))]
            + [("pred." + n, s) for n, s in kmax_predictor_shapes(K1)])


def kmax_packed_bytes(L: int, K1: int, layer_channels: Sequence[int]) -> int:
    """what axvs_kmax_decoder_packed_bytes returns: every slot rounded up to 256 bytes, the head first, then layer after layer"""
    slots = kmax_head_shapes(L, K1) + [s for cin in layer_channels for s in kmax_layer_shapes(cin, K1)]
    return sum((4 * math.prod(shape) + 255) // 256 * 256 for _, shape in slots)


def _kmax_affine(sd, p: str):
    """(a, c) of the BatchNorm `p`: a x + c"""
    a = sd[p + "weight"].double() / (sd[p + "running_var"].double() + KMAX_BN_EPS).sqrt()
    return a, sd[p + "bias"].double() - sd[p + "running_mean"].double() * a


def _kmax_convbn(sd, p: str):
    """(W [out, in * k], b [out]) of the ConvBN `p` with its norm (if it has one) folded in"""
    w = sd[p + "conv.weight"].double().flatten(1)
    b = sd[p + "conv.bias"].double() if p + "conv.bias" in sd else w.new_zeros(w.shape[0])
    if p + "norm.weight" in sd:
        a, c = _kmax_affine(sd, p + "norm.")
        w, b = w * a[:, None], b * a + c
    return w, b


def kmax_predictor_folded(sd, p: str) -> List[Tensor]:
    """AxvsKmaxPredictorParams of the kMaXPredictor `p`; the class bias carries add_bias_towards_void's constant"""
    dw_w, dw_b = _kmax_convbn(sd, p + "_pixel_space_head_conv0bnact.")
    cls_w, cls_b = _kmax_convbn(sd, p + "_transformer_class_head.")
    cls_b = cls_b.clone()
    cls_b[-1] += math.log((cls_b.numel() - 1) * 0.9 / (1 - 0.9))
    a, c = _kmax_affine(sd, p + "_pixel_space_mask_batch_norm.")
    return ([dw_w.t().contiguous(), dw_b, *_kmax_convbn(sd, p + "_pixel_space_head_conv1bnact."), *_kmax_convbn(sd, p + "_pixel_space_head_last_convbn."),
             *_kmax_convbn(sd, p + "_transformer_mask_head."), cls_w, cls_b, torch.cat([a, c, a.new_zeros(2)])])


def kmax_layer_folded(sd, p: str) -> List[Tensor]:
    """AxvsKmaxLayerParams of the kMaXTransformerLayer `p`.  kv: the value projection acts on the per-cluster SUM of the pixel-space rows
    (sum_p (A P_p + b) = A sum_p P_p + n b), under its own BatchNorm and `_kmeans_query_batch_norm_retrieved_value`; column 256 of kv_w
    multiplies the cluster's pixel count n."""
    vw, vb = _kmax_convbn(sd, p + "_pixel_v_conv_bn.")
    a, c = _kmax_affine(sd, p + "_kmeans_query_batch_norm_retrieved_value.")
    kv_w = torch.cat([vw * a[:, None], (vb * a)[:, None], vw.new_zeros(256, 3)], dim=1)
    sa, sc = _kmax_affine(sd, p + "_query_self_attention._batch_norm_similarity.")
    ra, rc = _kmax_affine(sd, p + "_query_self_attention._batch_norm_retrieved_value.")
    return ([*_kmax_convbn(sd, p + "_pixel_conv1_bn_act."), *_kmax_convbn(sd, p + "_query_conv1_bn_act.")] + kmax_predictor_folded(sd, p + "_predictor.")
            + [kv_w, c, *_kmax_convbn(sd, p + "_kmeans_query_conv3_bn."), *_kmax_convbn(sd, p + "_query_qkv_conv_bn."), torch.cat([sa, sc]),
               torch.cat([ra, rc]), *_kmax_convbn(sd, p + "_query_conv3_bn."), *_kmax_convbn(sd, p + "_query_ffn_conv1_bn_act."),
               *_kmax_convbn(sd, p + "_query_ffn_conv2_bn.")])


def kmax_head_folded(sd) -> List[Tensor]:
    """AxvsKmaxHeadParams of a MaXTronTransformerDecoder: `_cluster_centers.weight` is [256, L], the queries travel as rows [L, 256]"""
    return ([sd["_cluster_centers.weight"].double().t().contiguous(), *_kmax_convbn(sd, "_class_embedding_projection."),
             *_kmax_convbn(sd, "_mask_embedding_projection.")] + kmax_predictor_folded(sd, "_predictor."))


# ---- Video-kMaX's pixel decoder ---------------------------------------------------------------------------------------------------------
# AxvsKpixBlockParams / AxvsKpixFuseParams hold FOLDED float64 tensors as well (a slot the configuration does not have is None); the
# names are kMaXPixelDecoder's own state-dict names.
def kmax_pix_block_cin(in_channels0: int, dec_channels: Sequence[int], stage: int, j: int) -> int:
    return 4 * dec_channels[stage] if j > 0 else in_channels0 if stage == 0 else dec_channels[stage]


def kmax_pix_axis_shapes(b: int) -> List[tuple]:
    """(slot, shape) of AxvsKpixAxisParams, in order (_lib.KPIX_AXIS_FIELDS)"""
    return [("qkv_w", (4 * b, 2 * b)), ("qkv_b", (4 * b,)), ("eq", (509, b // 8)), ("ek", (509, b // 8)), ("ev", (509, b // 4)), ("sim_a", (24,)),
            ("out_ab", (3, 2 * b))]


def kmax_pix_block_shapes(cin: int, b: int, axial: bool) -> List[tuple]:
    """(slot, shape or None) of AxvsKpixBlockParams, in order (_lib.KPIX_BLOCK_FIELDS)"""
    mid, sc = (2 * b if axial else b), cin != 4 * b
    axis = kmax_pix_axis_shapes(b) if axial else [(n, None) for n, _ in kmax_pix_axis_shapes(b)]
    return ([("sc_w", (4 * b, cin) if sc else None), ("sc_b", (4 * b,) if sc else None), ("c1_w", (mid, cin)), ("c1_b", (mid,)),
             ("c2_w", None if axial else (9, b, b)), ("c2_b", None if axial else (b,))]
            + [("height." + n, s) for n, s in axis] + [("width." + n, s) for n, s in axis] + [("c3_w", (4 * b, mid)), ("c3_b", (4 * b,))])


def kmax_pix_fuse_shapes(low: int, high: int, b: int) -> List[tuple]:
    """(slot, shape or None) of AxvsKpixFuseParams, in order (_lib.KPIX_FUSE_FIELDS)"""
    return [("ln_w", (high,)), ("ln_b", (high,)), ("low_w", (b, low) if low != b else None), ("low_b", (b,) if low != b else None),
            ("high_w", (b, high) if high != b else None), ("high_b", (b,) if high != b else None)]


def kmax_pix_axis_folded(sd, p: str) -> List[Tensor]:
    """AxvsKpixAxisParams of the AxialAttention `p`: the qkv BatchNorm folded into the projection; of the similarity BatchNorm only the
    gains (its offsets are constant over the keys and cancel in the softmax); the retrieved-output BatchNorm as two gain rows and the
    sum of the two offset halves (the reference sums the two halves after the norm)."""
    w = sd[p + "qkv_transform.conv.weight"].double().flatten(1)
    a, c = _kmax_affine(sd, p + "_batch_norm_qkv.")
    sa, _ = _kmax_affine(sd, p + "_batch_norm_similarity.")
    ra, rc = _kmax_affine(sd, p + "_batch_norm_retrieved_output.")
    dv = ra.numel() // 2
    return [w * a[:, None], c, sd[p + "_query_rpe._embeddings.weight"].double(), sd[p + "_key_rpe._embeddings.weight"].double(),
            sd[p + "_value_rpe._embeddings.weight"].double(), sa, torch.stack([ra[:dv], ra[dv:], rc[:dv] + rc[dv:]])]


def kmax_pix_block_folded(sd, p: str) -> List[Optional[Tensor]]:
    """AxvsKpixBlockParams of the SingleBlock `p`; the 3 x 3 weight goes tap-major [9][out][in]"""
    sc = list(_kmax_convbn(sd, p + "_shortcut.")) if p + "_shortcut.conv.weight" in sd else [None, None]
    if p + "_conv2_bn_act.conv.weight" in sd:
        w, b = _kmax_convbn(sd, p + "_conv2_bn_act.")
        mid = [w.view(w.shape[0], -1, 9).permute(2, 0, 1).contiguous(), b] + [None] * 14
    else:
        mid = [None, None] + kmax_pix_axis_folded(sd, p + "_attention._height_axis.") + kmax_pix_axis_folded(sd, p + "_attention._width_axis.")
    return sc + list(_kmax_convbn(sd, p + "_conv1_bn_act.")) + mid + list(_kmax_convbn(sd, p + "_conv3_bn."))


def kmax_pix_fuse_folded(sd, index: int) -> List[Optional[Tensor]]:
    """AxvsKpixFuseParams of `_resized_fuses.{index}` with the LayerNorm of its high-resolution input, `_in_norms.{index + 1}`"""
    p = f"_resized_fuses.{index}."
    low = list(_kmax_convbn(sd, p + "_conv_bn_low.")) if p + "_conv_bn_low.conv.weight" in sd else [None, None]
    high = list(_kmax_convbn(sd, p + "_conv_bn_high.")) if p + "_conv_bn_high.conv.weight" in sd else [None, None]
    return [sd[f"_in_norms.{index + 1}.weight"].double(), sd[f"_in_norms.{index + 1}.bias"].double()] + low + high


# ---- ConvNeXt / ConvNeXtV2 backbone -------------------------------------------------------------------------------------------------------
# AxvsCnxDownParams / AxvsCnxBlockParams hold FOLDED float64 tensors in the kernels' layouts; the names are the reference ConvNeXt's own
# state-dict names.
def convnext_down_shapes(dims: Sequence[int], i: int) -> List[tuple]:
    """(slot, shape) of AxvsCnxDownParams for downsample layer i (0: the stem), in order (_lib.CNX_DOWN_FIELDS)"""
    ln, k = (dims[0], 48) if i == 0 else (dims[i - 1], 4 * dims[i - 1])
    return [("ln_w", (ln,)), ("ln_b", (ln,)), ("w", (dims[i], k)), ("b", (dims[i],))]


def convnext_block_shapes(dim: int, v2: bool) -> List[tuple]:
    """(slot, shape or None) of AxvsCnxBlockParams, in order (_lib.CNX_BLOCK_FIELDS)"""
    return [("dw_w", (49, dim)), ("dw_b", (dim,)), ("ln_w", (dim,)), ("ln_b", (dim,)), ("w1", (4 * dim, dim)), ("b1", (4 * dim,)),
            ("w2", (dim, 4 * dim)), ("b2", (dim,)), ("grn_gamma", (4 * dim,) if v2 else None)]


def convnext_down_folded(sd, i: int) -> List[Tensor]:
    """AxvsCnxDownParams of `downsample_layers.{i}`.  The stem (conv, then LayerNorm) keeps its weight's own (c, ky, kx) order: the gather
    kernel writes its patches in it.  Layers 1..3 (LayerNorm, then conv): the weight goes to the patch order (ky, kx, c)."""
    p = f"downsample_layers.{i}."
    conv, ln = (p + "0.", p + "1.") if i == 0 else (p + "1.", p + "0.")
    w = sd[conv + "weight"].double()
    w = w.flatten(1) if i == 0 else w.permute(0, 2, 3, 1).flatten(1)
    return [sd[ln + "weight"].double(), sd[ln + "bias"].double(), w.contiguous(), sd[conv + "bias"].double()]


def convnext_block_folded(sd, p: str) -> List[Optional[Tensor]]:
    """AxvsCnxBlockParams of the block `p`.  V1: the layer scale `gamma` (where the block has one) folded into pwconv2.  V2 (the block has
    `grn.gamma`): gamma (x Nx) + beta + x = x (1 + gamma Nx) + beta, so pwconv2's bias becomes W2 beta + b2 and the per-frame factor
    reaches the weight on the device."""
    w2, b2 = sd[p + "pwconv2.weight"].double(), sd[p + "pwconv2.bias"].double()
    grn = None
    if p + "grn.gamma" in sd:
        grn = sd[p + "grn.gamma"].double().flatten()
        # (a product and a row sum, not `@`: torch's first matrix product on a device allocates its BLAS workspace, 128 MiB that stay)
        b2 = (w2 * sd[p + "grn.beta"].double().flatten()[None, :]).sum(1) + b2
    elif p + "gamma" in sd:
        g = sd[p + "gamma"].double()
        w2, b2 = w2 * g[:, None], b2 * g
    dw = sd[p + "dwconv.weight"].double()
    return [dw.view(dw.shape[0], 49).t().contiguous(), sd[p + "dwconv.bias"].double(), sd[p + "norm.weight"].double(), sd[p + "norm.bias"].double(),
            sd[p + "pwconv1.weight"].double(), sd[p + "pwconv1.bias"].double(), w2.contiguous(), b2, grn]


# ---- ResNet bottleneck backbone -----------------------------------------------------------------------------------------------------------
# AxvsRnStemParams / AxvsRnBlockParams hold float64 tensors with every BatchNorm FOLDED, in the kernels' layouts; the names are the
# reference ResNet's own state-dict names (`<conv>.weight`, `<conv>.norm.{weight,bias,running_mean,running_var}`).
def resnet_block_shapes(cin: int, width: int, cout: int, shortcut: bool) -> List[tuple]:
    """(slot, shape or None) of AxvsRnBlockParams, in order (_lib.RN_BLOCK_FIELDS)"""
    return [("w1", (width, cin)), ("b1", (width,)), ("w2", (width, 9, width)), ("b2", (width,)), ("w3", (cout, width)), ("b3", (cout,)),
            ("ws", (cout, cin) if shortcut else None), ("bs", (cout,) if shortcut else None)]


def _resnet_conv_bn(sd, p: str, eps: float):
    """conv `p` behind its eval BatchNorm `p.norm` -> (weight scaled per output channel, bias), float64"""
    n = p + "norm."
    scale = sd[n + "weight"].double() / torch.sqrt(sd[n + "running_var"].double() + eps)
    return sd[p + "weight"].double() * scale[:, None, None, None], sd[n + "bias"].double() - sd[n + "running_mean"].double() * scale


def resnet_stem_folded(sd, eps: float) -> List[Tensor]:
    """AxvsRnStemParams of `stem.conv1`: w [147][C] ((colour, ky, kx) major, output channel fastest), b"""
    w, b = _resnet_conv_bn(sd, "stem.conv1.", eps)
    return [w.flatten(1).t().contiguous(), b]


def resnet_block_folded(sd, p: str, eps: float) -> List[Optional[Tensor]]:
    """AxvsRnBlockParams of the bottleneck block `p`: the 1x1 weights as matrices, the 3x3 weight as (output channel, tap, input channel);
    the block without `shortcut` has None in the last two slots"""
    w1, b1 = _resnet_conv_bn(sd, p + "conv1.", eps)
    w2, b2 = _resnet_conv_bn(sd, p + "conv2.", eps)
    w3, b3 = _resnet_conv_bn(sd, p + "conv3.", eps)
    ws, bs = (None, None)
    if p + "shortcut.weight" in sd:
        ws, bs = _resnet_conv_bn(sd, p + "shortcut.", eps)
        ws = ws.flatten(1).contiguous()
    return [w1.flatten(1).contiguous(), b1, w2.permute(0, 2, 3, 1).flatten(1, 2).contiguous(), b2, w3.flatten(1).contiguous(), b3, ws, bs]
