"""Video-kMaX's k-means query decoder on the device (eval-mode forward).

Reference (MaXTron_Video-kMaX): `MaXTronTransformerDecoder` with `kMaXTransformerLayer`, `AttentionOperation` and `kMaXPredictor`
(maxtron_deeplab/modeling/transformer_decoder/maxtron_transformer_decoder.py:49-231, 416-590), `ConvBN` / `get_norm` from
kmax_deeplab/modeling/pixel_decoder/kmax_pixel_decoder.py:32-72.  `MaXTronDeepLabHead.layers` calls it after the pixel decoder; its
outputs feed `CrossClipTrackingModule`, `match_clips` and `video_panoptic_inference`.

Per layer the reference builds the [B, L, T*h*w] mask logits to take an argmax over the clusters, scatters a one-hot tensor of that
size and contracts it with the [B, 256, T*h*w] values.  Here one kernel normalises a tile of pixels, contracts it with the mask kernels
on f32-input MFMAs and keeps a running (max, index): one int32 per pixel.  The cluster sums are a one-hot contraction over fixed
pixel chunks of a clip, reduced in chunk order -- no floating-point atomics, equal bits from run to run and between stacked and
single clips.  The value projection is applied to the sums (it is linear; the bias times the exact pixel count).  Equal maximal
logits go to the LOWER cluster index: torch's CPU rule for `max(dim)`; what the reference's GPU run does on exact ties is open.

Forward only: `train()` mode raises NotImplementedError at `forward` (SyncBN on batch statistics, DropPath and the auxiliary semantic head
are not part of the device path).  `aux_outputs` is returned as an empty list: the reference's `_set_aux_loss` interpolates every
layer's logits and pixel features to the final resolution in eval() too, where nobody reads them.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Mapping, Sequence

import torch
import torch.nn as nn
from torch import Tensor

from . import _lib
from ._params import kmax_head_folded, kmax_layer_folded
from .modules import _cached_pack, _dev_f32, _guarded, _pack_folded, _stream, _workspace_for

_BOTTLENECK, _KEY, _VALUE, _HEADS, _FFN, _MASK = 256, 128, 256, 8, 2048, 128


class _BN(nn.Module):
    """the state of a SyncBatchNorm(channels, eps=1e-3): an affine map on its running statistics in eval mode"""

    def __init__(self, channels: int):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(channels))
        self.bias = nn.Parameter(torch.zeros(channels))
        self.register_buffer("running_mean", torch.zeros(channels))
        self.register_buffer("running_var", torch.ones(channels))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))
        self.eps = 1e-3


class _Conv(nn.Module):
    def __init__(self, shape, bias: bool):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(shape))
        nn.init.trunc_normal_(self.weight, std=(2.0 / max(1, shape[1] * (shape[-1] if len(shape) == 4 else 1))) ** 0.5)
        if bias:
            self.bias = nn.Parameter(torch.zeros(shape[0]))


class _ConvBN(nn.Module):
    """the reference's ConvBN: `conv` (1-D or 2-D), `norm` (SyncBN or none); the activation has no state"""

    def __init__(self, cin: int, cout: int, dims: int, bias: bool = False, norm: bool = True, kernel: int = 1, depthwise: bool = False):
        super().__init__()
        self.conv = _Conv((cout, 1 if depthwise else cin) + (kernel,) * dims, bias)
        if norm:
            self.norm = _BN(cout)


class _Predictor(nn.Module):
    def __init__(self, num_classes_with_void: int):
        super().__init__()
        self._pixel_space_head_conv0bnact = _ConvBN(256, 256, 2, kernel=5, depthwise=True)
        self._pixel_space_head_conv1bnact = _ConvBN(256, 256, 2)
        self._pixel_space_head_last_convbn = _ConvBN(256, _MASK, 2, bias=True)
        self._transformer_mask_head = _ConvBN(256, _MASK, 1)
        self._transformer_class_head = _ConvBN(256, num_classes_with_void, 1, bias=True, norm=False)
        self._pixel_space_mask_batch_norm = _BN(1)
        nn.init.constant_(self._pixel_space_mask_batch_norm.weight, 0.1)


class _Attention(nn.Module):
    def __init__(self):
        super().__init__()
        self._batch_norm_similarity = _BN(_HEADS)
        self._batch_norm_retrieved_value = _BN(_VALUE)


class _Layer(nn.Module):
    def __init__(self, in_channel_pixel: int, num_classes_with_void: int):
        super().__init__()
        self._query_conv1_bn_act = _ConvBN(256, _BOTTLENECK, 1)
        self._pixel_conv1_bn_act = _ConvBN(in_channel_pixel, _BOTTLENECK, 2)
        self._query_qkv_conv_bn = _ConvBN(_BOTTLENECK, 2 * _KEY + _VALUE, 1)
        self._pixel_v_conv_bn = _ConvBN(_BOTTLENECK, _VALUE, 2)
        self._query_self_attention = _Attention()
        self._query_conv3_bn = _ConvBN(_VALUE, 256, 1)
        self._query_ffn_conv1_bn_act = _ConvBN(256, _FFN, 1)
        self._query_ffn_conv2_bn = _ConvBN(_FFN, 256, 1)
        self._predictor = _Predictor(num_classes_with_void)
        self._kmeans_query_batch_norm_retrieved_value = _BN(_VALUE)
        self._kmeans_query_conv3_bn = _ConvBN(_VALUE, 256, 1)


def _check_config(dec_layers: Sequence[int], in_channels: Sequence[int], num_classes: int, num_queries: int, num_clip_frames: int) -> None:
    if len(dec_layers) != 3 or len(in_channels) != 3 or any(int(n) < 0 for n in dec_layers) or not 1 <= sum(dec_layers) <= 16:
        raise NotImplementedError(f"axial_vs_amd: the decoder kernels take 1..16 layers over 3 levels (dec_layers {list(dec_layers)})")
    if any(int(c) % 16 or not 16 <= int(c) <= 2048 for c in in_channels):
        raise NotImplementedError(f"axial_vs_amd: in_channels {list(in_channels)} must be multiples of 16 in 16..2048")
    if not 1 <= num_queries <= 256:
        raise NotImplementedError(f"axial_vs_amd: the decoder kernels take 1..256 queries (got {num_queries})")
    if not 1 <= num_classes + 1 <= 256:
        raise NotImplementedError(f"axial_vs_amd: the decoder kernels take at most 255 classes (got {num_classes})")
    if not 1 <= num_clip_frames <= 16:
        raise NotImplementedError(f"axial_vs_amd: the decoder kernels take clips of 1..16 frames (got {num_clip_frames})")


def filter_training_keys(state_dict: Mapping[str, Tensor]) -> Dict[str, Tensor]:
    """A checkpoint's decoder state without the `_auxiliary_semantic_predictor.*` tensors (training only): what
    `KMaXTransformerDecoder.load_state_dict(strict=True)` takes."""
    return {k: v for k, v in state_dict.items() if not k.startswith("_auxiliary_semantic_predictor.")}


def _cfg(B: int, T: int, L: int, K1: int, dec_layers, in_channels, sizes, pan, want_masks=True, want_pixel_feature=True) -> _lib.AxvsKmaxCfg:
    levels = [l for l, n in enumerate(dec_layers) for _ in range(int(n))]
    return _lib.AxvsKmaxCfg(B=B, T=T, L=L, K1=K1, num_layers=len(levels), layer_level=(C.c_int * 16)(*levels),
                            in_channels=(C.c_int * 3)(*[int(c) for c in in_channels]), h=(C.c_int * 3)(*[int(s[0]) for s in sizes]),
                            w=(C.c_int * 3)(*[int(s[1]) for s in sizes]), pan_channels=int(pan[0]), H=int(pan[1]), W=int(pan[2]), heads=_HEADS,
                            base_filters=_KEY, want_masks=int(want_masks), want_pixel_feature=int(want_pixel_feature))


def _pack(sd: Mapping[str, Tensor], dec_layers, in_channels, L: int, K1: int) -> Tensor:
    """fold (float64) and pack: one blob of fp32 tensors in the kernels' layouts"""
    sd = {k: v.detach() for k, v in sd.items()}
    layers = (kmax_layer_folded(sd, f"_kmax_transformer_layers.{i}.") for i in range(sum(int(n) for n in dec_layers)))
    return _pack_folded("axvs_kmax_decoder", _cfg(1, 1, L, K1, dec_layers, in_channels, [(1, 1)] * 3, (256, 1, 1)),
                        [(_lib.AxvsKmaxLayerParams, layers), (_lib.AxvsKmaxHeadParams, [kmax_head_folded(sd)])])


def _clips(BT: int, num_clip_frames: int, cross_clip_training: bool):
    B = BT // num_clip_frames if cross_clip_training else 1
    if B < 1 or BT % B:
        raise RuntimeError(f"axial_vs_amd: {BT} frames do not divide into clips of {num_clip_frames}")
    return B, BT // B


def _inputs(x: Sequence[Tensor], panoptic_features: Tensor, in_channels):
    if len(x) != 3:
        raise RuntimeError(f"axial_vs_amd: the decoder takes three feature levels (got {len(x)})")
    feats = [_dev_f32(f, "x") for f in x]
    pan = _dev_f32(panoptic_features, "panoptic_features")
    BT = feats[0].shape[0]
    for f, c in zip(feats, in_channels):
        if f.dim() != 4 or f.shape[0] != BT or f.shape[1] != c:
            raise RuntimeError(f"axial_vs_amd: feature {tuple(f.shape)} must be [{BT}, {c}, h, w]")
    if pan.dim() != 4 or pan.shape[0] != BT or pan.shape[1] != 256:
        raise RuntimeError(f"axial_vs_amd: panoptic_features {tuple(pan.shape)} must be [{BT}, 256, H, W]")
    return feats, pan


def _run(packed: Tensor, feats, pan, B, T, L, K1, dec_layers, in_channels, want_masks, want_pixel_feature, return_index_maps):
    Lb, dev = _lib.lib(), pan.device
    sizes = [tuple(f.shape[-2:]) for f in feats]
    H, W = pan.shape[-2:]
    cfg = _cfg(B, T, L, K1, dec_layers, in_channels, sizes, (256, H, W), want_masks, want_pixel_feature)
    st = _stream(dev)
    ws = _workspace_for("axvs_kmax_decoder_workspace_bytes", dev, st, C.byref(cfg))
    f32 = dict(dtype=torch.float32, device=dev)
    logits = torch.empty(B, L, K1, **f32)
    masks = torch.empty(B, L, T, H, W, **f32) if want_masks else None
    emb = torch.empty(B, L, _MASK, **f32)
    pix = torch.empty(B, _MASK, T, H, W, **f32) if want_pixel_feature else None
    centers = torch.empty(B, L, 256, **f32)
    levels = [l for l, n in enumerate(dec_layers) for _ in range(int(n))]
    counts = [B * T * sizes[l][0] * sizes[l][1] for l in levels]
    dbg = torch.empty(sum(counts), dtype=torch.int32, device=dev) if return_index_maps else None
    ptr = lambda t: None if t is None else t.data_ptr()
    fp = (C.c_void_p * 3)(*[f.data_ptr() for f in feats])
    _lib.check(Lb.axvs_kmax_decoder_fwd(C.byref(cfg), packed.data_ptr(), fp, pan.data_ptr(), logits.data_ptr(), ptr(masks), emb.data_ptr(), ptr(pix),
                                        centers.data_ptr(), ptr(dbg), ws.data_ptr(), ws.numel(), st), "axvs_kmax_decoder_fwd")
    out = {"pred_logits": logits, "pred_masks": masks, "pred_mask_embeddings": emb, "pixel_feature": pix, "aux_outputs": [],
           "cluster_centers": centers}
    if return_index_maps:
        maps, o = [], 0
        for n in counts:
            maps.append(dbg[o:o + n].view(B, n // B))
            o += n
        out["index_maps"] = maps
    return out


@torch.no_grad()
def kmax_decoder_forward(params: Mapping[str, Tensor], x: Sequence[Tensor], panoptic_features: Tensor, dec_layers: Sequence[int],
                         num_clip_frames: int, cross_clip_training: bool = False, pred_masks: bool = True, pixel_feature: bool = True,
                         return_index_maps: bool = False) -> dict:
    """The decoder's eval forward from a mapping of the reference's state-dict names (`_auxiliary_semantic_predictor.*` ignored) to GPU
    tensors.  Folds and packs the parameters on every call: `KMaXTransformerDecoder` keeps the packed weights."""
    in_channels = [params[f"_kmax_transformer_layers.{sum(dec_layers[:l])}._pixel_conv1_bn_act.conv.weight"].shape[1] if dec_layers[l] else 16
                   for l in range(3)]
    L = params["_cluster_centers.weight"].shape[1]
    K1 = params["_predictor._transformer_class_head.conv.weight"].shape[0]
    _check_config(dec_layers, in_channels, K1 - 1, L, num_clip_frames)
    feats, pan = _inputs(x, panoptic_features, in_channels)
    B, T = _clips(feats[0].shape[0], num_clip_frames, cross_clip_training)
    with torch.cuda.device(pan.device):
        packed = _pack(params, dec_layers, in_channels, L, K1)
        return _run(packed, feats, pan, B, T, L, K1, dec_layers, in_channels, pred_masks, pixel_feature, return_index_maps)


class KMaXTransformerDecoder(nn.Module):
    """`MaXTronTransformerDecoder` under the reference's own parameter and buffer names: a checkpoint's decoder state loads with
    `load_state_dict(filter_training_keys(sd), strict=True)`.

    forward(x, panoptic_features, semantic_features=None) -> the reference's dict:
        pred_logits [B,L,K+1], pred_masks [B,L,T,H,W], pred_mask_embeddings [B,L,128], pixel_feature [B,128,T,H,W],
        cluster_centers [B,L,256], aux_outputs [] (always empty: see the module docstring).
    x: three levels [(B T), C_l, h_l, w_l] at strides 32 / 16 / 8; panoptic_features [(B T), 256, H, W].  B = BT // num_clip_frames with
    `cross_clip_training`, else 1; T = BT // B.  `return_pred_masks` / `return_pixel_feature` (attributes, default True) switch the two
    full-resolution outputs off: the entry is then None.  Equal maximal logits go to the lower cluster index.  GPU tensors only;
    eval() only; runs on the current stream; the folded weights are packed once and again when a parameter or running statistic changes."""

    def __init__(self, dec_layers: Sequence[int], in_channels: Sequence[int], num_classes: int, num_queries: int, num_clip_frames: int,
                 cross_clip_training: bool = False):
        super().__init__()
        _check_config(dec_layers, in_channels, num_classes, num_queries, num_clip_frames)
        self._num_blocks = [int(n) for n in dec_layers]
        self._in_channels = [int(c) for c in in_channels]
        self._kmax_transformer_layers = nn.ModuleList(
            [_Layer(self._in_channels[l], num_classes + 1) for l in range(3) for _ in range(self._num_blocks[l])])
        self._num_queries, self._num_classes = int(num_queries), int(num_classes)
        self._cluster_centers = nn.Embedding(256, num_queries)
        self._class_embedding_projection = _ConvBN(256, 256, 1)
        self._mask_embedding_projection = _ConvBN(256, 256, 1)
        self._predictor = _Predictor(num_classes + 1)
        self._num_clip_frames, self._cross_clip_training = int(num_clip_frames), bool(cross_clip_training)
        self.return_pred_masks = self.return_pixel_feature = True

    def _state(self) -> Dict[str, Tensor]:
        sd = dict(self.named_parameters())
        sd.update(self.named_buffers())
        return sd

    def _packed(self) -> Tensor:
        return _cached_pack(self, "kmax", "f32", (self,), lambda dt: _pack(self._state(), self._num_blocks, self._in_channels, self._num_queries,
                                                                           self._num_classes + 1), buffers=True)

    def _stage_cfg(self, index: int, feature: Tensor):
        l = [l for l, n in enumerate(self._num_blocks) for _ in range(n)][index]
        B, T = _clips(feature.shape[0], self._num_clip_frames, self._cross_clip_training)
        sizes = [(1, 1)] * 3
        sizes[l] = tuple(feature.shape[-2:])
        if feature.dim() != 4 or feature.shape[1] != self._in_channels[l]:
            raise RuntimeError(f"axial_vs_amd: feature {tuple(feature.shape)} must be [(B T), {self._in_channels[l]}, h, w]")
        return _cfg(B, T, self._num_queries, self._num_classes + 1, self._num_blocks, self._in_channels, sizes, (256, 1, 1)), B, T

    @_guarded
    @torch.no_grad()
    def forward(self, x: Sequence[Tensor], panoptic_features: Tensor, semantic_features=None, return_index_maps: bool = False) -> dict:
        """`return_index_maps=True` (a debugging aid, what the tests read) adds `index_maps`: every layer's int32 [B, T*h*w] cluster
        index per pixel, as the layer consumed it."""
        if self.training:
            raise NotImplementedError("axial_vs_amd: KMaXTransformerDecoder has a forward-only HIP path -- call .eval() (batch-statistics SyncBN, "
                                      "DropPath and the auxiliary semantic head are not part of it)")
        feats, pan = _inputs(x, panoptic_features, self._in_channels)
        B, T = _clips(feats[0].shape[0], self._num_clip_frames, self._cross_clip_training)
        return _run(self._packed(), feats, pan, B, T, self._num_queries, self._num_classes + 1, self._num_blocks, self._in_channels,
                    self.return_pred_masks, self.return_pixel_feature, return_index_maps)

    @_guarded
    @torch.no_grad()
    def assign(self, query: Tensor, feature: Tensor, index: int):
        """The assignment of layer `index`: query [B,L,256] (rows; the reference's query_feature transposed), feature [(B T),C_l,h,w] of
        the layer's level -> (index map int32 [B, T*h*w], the layer's class logits [B,L,K+1])."""
        q, f = _dev_f32(query, "query"), _dev_f32(feature, "feature")
        cfg, B, T = self._stage_cfg(index, f)
        Lb, dev, L = _lib.lib(), f.device, self._num_queries
        if q.shape != (B, L, 256):
            raise RuntimeError(f"axial_vs_amd: query {tuple(q.shape)} must be [{B}, {L}, 256]")
        packed = self._packed()
        st = _stream(dev)
        ws = _workspace_for("axvs_kmax_stage_workspace_bytes", dev, st, C.byref(cfg), index, 0)
        idx = torch.empty(B, T * f.shape[-2] * f.shape[-1], dtype=torch.int32, device=dev)
        cls = torch.empty(B, L, self._num_classes + 1, dtype=torch.float32, device=dev)
        _lib.check(Lb.axvs_kmax_assign_fwd(C.byref(cfg), packed.data_ptr(), index, q.data_ptr(), f.data_ptr(), idx.data_ptr(), cls.data_ptr(), ws.data_ptr(),
                                           ws.numel(), st), "axvs_kmax_assign_fwd")
        return idx, cls

    @_guarded
    @torch.no_grad()
    def layer(self, query: Tensor, feature: Tensor, index_map: Tensor, index: int) -> Tensor:
        """Layer `index` given its index map (int32 [B, T*h*w]; an index outside 0..L-1 joins no cluster) -> the new query feature [B,L,256]."""
        q, f = _dev_f32(query, "query"), _dev_f32(feature, "feature")
        cfg, B, T = self._stage_cfg(index, f)
        Lb, dev, L = _lib.lib(), f.device, self._num_queries
        S = T * f.shape[-2] * f.shape[-1]
        if q.shape != (B, L, 256) or index_map.shape != (B, S) or index_map.dtype != torch.int32 or not index_map.is_cuda:
            raise RuntimeError(f"axial_vs_amd: query {tuple(q.shape)}, index_map {tuple(index_map.shape)} must be [{B}, {L}, 256], GPU int32 [{B}, {S}]")
        index_map = index_map.contiguous()
        packed = self._packed()
        st = _stream(dev)
        ws = _workspace_for("axvs_kmax_stage_workspace_bytes", dev, st, C.byref(cfg), index, 1)
        out = torch.empty(B, L, 256, dtype=torch.float32, device=dev)
        _lib.check(Lb.axvs_kmax_layer_fwd(C.byref(cfg), packed.data_ptr(), index, q.data_ptr(), f.data_ptr(), index_map.data_ptr(), out.data_ptr(),
                                          ws.data_ptr(), ws.numel(), st), "axvs_kmax_layer_fwd")
        return out
