"""Video-kMaX's pixel decoder on the device (eval-mode forward), and the head that chains it between the within-clip module and the
k-means query decoder.

Reference (MaXTron_Video-kMaX): `kMaXPixelDecoder` with `BlockGroup` / `SingleBlock`, `AxialAttention2D` / `AxialAttention`,
`RelativePositionalEncoding`, `ResizedFuse` and `ConvBN` (kmax_deeplab/modeling/pixel_decoder/kmax_pixel_decoder.py:32-371), the
channels-first `LayerNorm` of kmax_deeplab/modeling/backbone/convnext.py:52-80, and `MaXTronDeepLabHead`
(maxtron_deeplab/modeling/meta_arch/maxtron_deeplab_head.py:25-92).

Per axis pass the reference builds a [N, 24, L, L] similarity tensor and gathers three [L, L, d] relative-position tables.  Here one
kernel per axis pass owns up to 64 queries of a (sequence, head): the position terms are Toeplitz in (query, key), so they are
contractions with a window of the [509, d] table read back along the skew; the similarity BatchNorm's offsets cancel in the softmax and
its gains, like those of the retrieved-output BatchNorm, are applied in the kernel.  1x1 convolutions run on the split-precision GEMM
with their BatchNorms folded in, the 3x3 convolutions as an fp32 implicit GEMM.  Frames are independent: nothing mixes the batch axis.

Forward only: `train()` mode raises NotImplementedError at `forward_features` (SyncBN on batch statistics and DropPath are not part of
the device path).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Mapping, Sequence

import torch
import torch.nn as nn
from torch import Tensor

from . import _lib
from ._params import kmax_pix_block_cin, kmax_pix_block_folded, kmax_pix_fuse_folded
from .kmax_decoder import _BN, _ConvBN
from .modules import _cached_pack, _dev_f32, _on, _pack_folded, _stream, _workspace_for

_HEADS, _TABLE, _STRIDES = 8, 509, (32, 16, 8, 4)
_LDS_BYTES = 160 * 1024


def _attn_lds_bytes(L: int, b: int) -> int:
    """the LDS plan of the attention kernel (csrc/axvs_kmax_pix.h: kpix_attn_lds) for axis length L at base filter b"""
    L16 = (L + 15) // 16 * 16
    qb = min(64, L16)
    nw, dk, dv = L16 + qb, b // 8, b // 4
    return 4 * (qb * (L16 + 4) + 4 * 2 * 16 * 33 + max((qb + L16 + 2 * nw) * (dk + 4), (L16 + nw) * (dv + 4)))


def max_axis_length(base_filter: int) -> int:
    """the longest axis the attention kernel takes at this base filter: 128, or what 160 KiB of LDS hold (80 at base filter 512)"""
    return max(L for L in range(1, 129) if _attn_lds_bytes(L, base_filter) <= _LDS_BYTES)


def query_shapes(spatial_shape: Sequence[int]):
    """the reference's query_shape per stage: spatial_shape // stride + spatial_shape % 2"""
    H, W = int(spatial_shape[0]), int(spatial_shape[1])
    return [(H // s + H % 2, W // s + W % 2) for s in _STRIDES]


def _check_config(in_channels, dec_layers, dec_channels, layer_types) -> None:
    if not (len(in_channels) == len(dec_layers) == len(dec_channels) == len(layer_types) == 4):
        raise NotImplementedError(f"axial_vs_amd: the pixel decoder kernels take four stages (got {len(in_channels)} features, dec_layers "
                                  f"{list(dec_layers)}, dec_channels {list(dec_channels)}, layer_types {list(layer_types)})")
    for i, (c, n, b, t) in enumerate(zip(in_channels, dec_layers, dec_channels, layer_types)):
        if int(c) % 16 or not 16 <= int(c) <= 2048:
            raise NotImplementedError(f"axial_vs_amd: in_channels {list(in_channels)} must be multiples of 16 in 16..2048")
        if not 1 <= int(n) <= 16:
            raise NotImplementedError(f"axial_vs_amd: the pixel decoder kernels take 1..16 blocks per stage (dec_layers {list(dec_layers)})")
        if str(t).lower() == "axial":
            if int(b) not in (512, 256, 128):
                raise NotImplementedError(f"axial_vs_amd: an axial stage's base filter must be 512, 256 or 128 (stage {i}: {b})")
        elif str(t).lower() == "bottleneck":
            if int(b) % 32 or not 32 <= int(b) <= 256:
                raise NotImplementedError(f"axial_vs_amd: a bottleneck stage's base filter must be a multiple of 32 up to 256 (stage {i}: {b})")
        else:
            raise NotImplementedError(f"axial_vs_amd: layer type {t!r} is neither 'axial' nor 'bottleneck'")


def _check_axes(sizes, dec_channels, layer_types) -> None:
    for i, ((h, w), b, t) in enumerate(zip(sizes, dec_channels, layer_types)):
        if str(t).lower() == "axial" and max(h, w) > max_axis_length(int(b)):
            raise NotImplementedError(f"axial_vs_amd: stage {i}: axis length {max(h, w)} is past the attention kernel's bound at base filter {b} "
                                      f"(at most {max_axis_length(int(b))}: 128, or what 160 KiB of LDS hold)")


def _cfg(N: int, in_channels, sizes, dec_layers, dec_channels, layer_types) -> _lib.AxvsKpixCfg:
    i4 = C.c_int * 4
    return _lib.AxvsKpixCfg(N=N, in_channels=i4(*[int(c) for c in in_channels]), h=i4(*[int(s[0]) for s in sizes]), w=i4(*[int(s[1]) for s in sizes]),
                            base=i4(*[int(b) for b in dec_channels]), blocks=i4(*[int(n) for n in dec_layers]),
                            axial=i4(*[int(str(t).lower() == "axial") for t in layer_types]), heads=_HEADS)


def _pack(sd: Mapping[str, Tensor], in_channels, dec_layers, dec_channels, layer_types) -> Tensor:
    """fold (float64) and pack: one blob of fp32 tensors in the kernels' layouts"""
    sd = {k: v.detach() for k, v in sd.items()}
    blocks = (kmax_pix_block_folded(sd, f"_stages.{i}._blocks.{j}.") for i in range(4) for j in range(int(dec_layers[i])))
    fuses = (kmax_pix_fuse_folded(sd, i) for i in range(3))
    return _pack_folded("axvs_kmax_pix", _cfg(1, in_channels, [(1, 1)] * 4, dec_layers, dec_channels, layer_types),
                        [(_lib.AxvsKpixBlockParams, blocks), (_lib.AxvsKpixFuseParams, fuses)], extra=[sd["_in_norms.0.weight"], sd["_in_norms.0.bias"]])


def _features(feats: Sequence[Tensor], in_channels) -> list:
    if len(feats) != 4:
        raise RuntimeError(f"axial_vs_amd: the pixel decoder takes four feature levels (got {len(feats)})")
    out = [_dev_f32(f, "features") for f in feats]
    N = out[0].shape[0]
    for f, c in zip(out, in_channels):
        if f.dim() != 4 or f.shape[0] != N or f.shape[1] != c:
            raise RuntimeError(f"axial_vs_amd: feature {tuple(f.shape)} must be [{N}, {c}, h, w]")
    return out


def _check_sizes(feats, spatial_shape) -> None:
    sizes, want = [tuple(f.shape[-2:]) for f in feats], query_shapes(spatial_shape)
    if len(feats) == 4 and sizes != want:
        raise NotImplementedError(f"axial_vs_amd: feature sizes {sizes} must equal query_shape {want} of spatial_shape {tuple(spatial_shape)} "
                                  "(spatial_shape // stride + spatial_shape % 2): the relative-position tables are built for it")


def _run(packed: Tensor, feats, in_channels, dec_layers, dec_channels, layer_types, spatial_shape):
    sizes = [tuple(f.shape[-2:]) for f in feats]
    _check_axes(sizes, dec_channels, layer_types)
    dev, N = feats[0].device, feats[0].shape[0]
    cfg = _cfg(N, in_channels, sizes, dec_layers, dec_channels, layer_types)
    st = _stream(dev)
    ws = _workspace_for("axvs_kmax_pix_workspace_bytes", dev, st, C.byref(cfg))
    outs = [torch.empty(N, 4 * int(b), h, w, dtype=torch.float32, device=dev) for b, (h, w) in zip(dec_channels, sizes)]
    fp = (C.c_void_p * 4)(*[f.data_ptr() for f in feats])
    op = (C.c_void_p * 4)(*[o.data_ptr() for o in outs])
    _lib.check(_lib.lib().axvs_kmax_pix_decoder_fwd(C.byref(cfg), packed.data_ptr(), fp, op, ws.data_ptr(), ws.numel(), st), "axvs_kmax_pix_decoder_fwd")
    return outs


def _ordered(features) -> list:
    """a mapping of feature names (res5 .. res2: coarsest = greatest name) or a sequence, coarsest first"""
    if isinstance(features, Mapping):
        return [features[k] for k in sorted(features, reverse=True)]
    return list(features)


@torch.no_grad()
def kmax_pixel_decoder_forward(params: Mapping[str, Tensor], features, dec_layers: Sequence[int], dec_channels: Sequence[int],
                               layer_types: Sequence[str], spatial_shape: Sequence[int]):
    """The pixel decoder's eval forward from a mapping of the reference's state-dict names to GPU tensors.  `features`: a mapping whose
    names sort from the finest to the coarsest level (res2 .. res5), or a sequence coarsest first.  Folds and packs the parameters on every
    call: `KMaXPixelDecoder` keeps the packed weights.  -> (panoptic_features, semantic_features, multi_scale_features)."""
    raw = _ordered(features)
    in_channels = [int(params[f"_in_norms.{i}.weight"].shape[0]) for i in range(len(raw))]
    _check_config(in_channels, dec_layers, dec_channels, layer_types)
    _check_sizes(raw, spatial_shape)
    feats = _features(raw, in_channels)
    with _on(feats[0].device):
        packed = _pack(params, in_channels, dec_layers, dec_channels, layer_types)
        outs = _run(packed, feats, in_channels, dec_layers, dec_channels, layer_types, spatial_shape)
    return outs[-1], [raw[0], raw[2], raw[3]], outs[:3]


class _LayerNorm(nn.Module):
    """the state of the reference's channels-first LayerNorm (eps 1e-6)"""

    def __init__(self, channels: int):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(channels))
        self.bias = nn.Parameter(torch.zeros(channels))


class _RPE(nn.Module):
    def __init__(self, depth: int):
        super().__init__()
        self._embeddings = nn.Embedding(_TABLE, depth)
        nn.init.trunc_normal_(self._embeddings.weight, std=1.0)


class _AxialAttention(nn.Module):
    def __init__(self, in_planes: int, key_depth: int, value_depth: int):
        super().__init__()
        self.qkv_transform = _ConvBN(in_planes, 2 * key_depth + value_depth, 1, norm=False)
        self._query_rpe = _RPE(key_depth // _HEADS)
        self._key_rpe = _RPE(key_depth // _HEADS)
        self._value_rpe = _RPE(value_depth // _HEADS)
        self._batch_norm_qkv = _BN(2 * key_depth + value_depth)
        self._batch_norm_similarity = _BN(3 * _HEADS)
        self._batch_norm_retrieved_output = _BN(2 * value_depth)


class _AxialAttention2D(nn.Module):
    def __init__(self, in_planes: int, filters: int):
        super().__init__()
        self._height_axis = _AxialAttention(in_planes, filters, 2 * filters)
        self._width_axis = _AxialAttention(2 * filters, filters, 2 * filters)


class _SingleBlock(nn.Module):
    def __init__(self, inplanes: int, base: int, axial: bool):
        super().__init__()
        mid = 2 * base if axial else base
        self._conv1_bn_act = _ConvBN(inplanes, mid, 2)
        if axial:
            self._attention = _AxialAttention2D(mid, base)
        else:
            self._conv2_bn_act = _ConvBN(base, base, 2, kernel=3)
        self._conv3_bn = _ConvBN(mid, 4 * base, 2)
        nn.init.zeros_(self._conv3_bn.norm.weight)          # the reference's norm_init = 0.0
        if inplanes != 4 * base:
            self._shortcut = _ConvBN(inplanes, 4 * base, 2)


class _BlockGroup(nn.Module):
    def __init__(self, inplanes: int, base: int, num_blocks: int, axial: bool):
        super().__init__()
        self._blocks = nn.ModuleList([_SingleBlock(inplanes if j == 0 else 4 * base, base, axial) for j in range(num_blocks)])


class _ResizedFuse(nn.Module):
    def __init__(self, low: int, high: int, out: int):
        super().__init__()
        if low != out:
            self._conv_bn_low = _ConvBN(low, out, 2)
        if high != out:
            self._conv_bn_high = _ConvBN(high, out, 2)


class KMaXPixelDecoder(nn.Module):
    """`kMaXPixelDecoder` under the reference's own parameter and buffer names: a checkpoint's `pixel_decoder.*` state loads with
    `load_state_dict(strict=True)`.

    input_shape: feature name -> an object with `channels` and `stride` (four levels).  forward_features(features) ->
    (panoptic_features [N, 4 dec_channels[3], h3, w3], semantic_features = the caller's own [res5, res3, res2] tensors,
    multi_scale_features = the outputs of stages 0..2), all NCHW fp32.  Every feature map must have the size `query_shape` of its stage
    (spatial_shape // stride + spatial_shape % 2), as in the reference.  GPU tensors only; eval() only; runs on the current stream; the
    folded weights are packed once and again when a parameter or running statistic changes (`invalidate_pack` forgets them).
    Bounds (NotImplementedError outside them): four stages of 1..16 blocks; axial stages with base filter 512, 256 or 128 and axis
    lengths up to `max_axis_length(base filter)`; bottleneck stages with base filter a multiple of 32 up to 256; in_channels multiples
    of 16 up to 2048."""

    def __init__(self, input_shape, dec_layers: Sequence[int], dec_channels: Sequence[int], layer_types: Sequence[str], spatial_shape: Sequence[int],
                 drop_path_prob: float = 0.0):
        super().__init__()
        levels = sorted(input_shape.items(), key=lambda kv: -kv[1].stride)
        self.in_features = [k for k, _ in levels]
        self._in_channels = [int(v.channels) for _, v in levels]
        _check_config(self._in_channels, dec_layers, dec_channels, layer_types)
        self.num_stages = 4
        self._dec_layers, self._dec_channels = [int(n) for n in dec_layers], [int(b) for b in dec_channels]
        self._layer_types = [str(t).lower() for t in layer_types]
        self._spatial_shape = (int(spatial_shape[0]), int(spatial_shape[1]))
        self.drop_path_prob = float(drop_path_prob)         # (training only: the device path is the eval forward)
        _check_axes(query_shapes(self._spatial_shape), self._dec_channels, self._layer_types)
        self._in_norms = nn.ModuleList([_LayerNorm(c) for c in self._in_channels])
        self._stages = nn.ModuleList([_BlockGroup(self._in_channels[0] if i == 0 else self._dec_channels[i], self._dec_channels[i], self._dec_layers[i],
                                                  self._layer_types[i] == "axial") for i in range(4)])
        self._resized_fuses = nn.ModuleList([_ResizedFuse(4 * self._dec_channels[i - 1], self._in_channels[i], self._dec_channels[i]) for i in range(1, 4)])

    def _state(self) -> Dict[str, Tensor]:
        sd = dict(self.named_parameters())
        sd.update(self.named_buffers())
        return sd

    def _config(self):
        return self._in_channels, self._dec_layers, self._dec_channels, self._layer_types

    def _packed(self) -> Tensor:
        return _cached_pack(self, "kpix", "f32", (self,), lambda dt: _pack(self._state(), *self._config()), buffers=True)

    def _require_eval(self) -> None:
        if self.training:
            raise NotImplementedError("axial_vs_amd: KMaXPixelDecoder has a forward-only HIP path -- call .eval() (batch-statistics SyncBN and "
                                      "DropPath are not part of it)")

    @torch.no_grad()
    def forward_features(self, features: Mapping[str, Tensor]):
        self._require_eval()
        raw = [features[k] for k in self.in_features]
        _check_sizes(raw, self._spatial_shape)
        feats = _features(raw, self._in_channels)
        with _on(feats[0].device):
            outs = _run(self._packed(), feats, *self._config(), self._spatial_shape)
        return outs[-1], [raw[0], raw[2], raw[3]], outs[:3]

    # ---- stage entries (what the tests read): any map size inside the kernels' bounds, not only the stage's query_shape -------------------
    def _stage_cfg(self, sizes: Dict[int, tuple], N: int):
        full = [sizes.get(i, (1, 1)) for i in range(4)]
        _check_axes(full, self._dec_channels, self._layer_types)
        return _cfg(N, *self._config()[:1], full, *self._config()[1:])

    def _locate(self, stage: int, index: int) -> int:
        if not (0 <= stage < 4 and 0 <= index < self._dec_layers[stage]):
            raise IndexError(f"axial_vs_amd: stage {stage} has no block {index}")
        return sum(self._dec_layers[:stage]) + index

    @torch.no_grad()
    def axial_attn(self, qkv: Tensor, stage: int, index: int, axis: int) -> Tensor:
        """One axis pass (0: over the columns of a frame, length h; 1: over its rows) of block `index` of `stage` on qkv rows
        [N, h, w, 4 b] (channels-last, after the qkv BatchNorm) -> [N, h, w, 2 b]: the retrieved output after its BatchNorm."""
        self._require_eval()
        q = _dev_f32(qkv, "qkv")
        b = self._dec_channels[stage]
        if self._layer_types[stage] != "axial" or q.dim() != 4 or q.shape[3] != 4 * b:
            raise RuntimeError(f"axial_vs_amd: qkv {tuple(q.shape)} must be [N, h, w, {4 * b}] of an axial stage")
        N, h, w = q.shape[:3]
        with _on(q.device):
            cfg = self._stage_cfg({stage: (h, w)}, N)
            out = torch.empty(N, h, w, 2 * b, dtype=torch.float32, device=q.device)
            _lib.check(_lib.lib().axvs_kmax_pix_axial_attn_fwd(C.byref(cfg), self._packed().data_ptr(), self._locate(stage, index), int(axis), q.data_ptr(),
                                                               out.data_ptr(), _stream(q.device)), "axvs_kmax_pix_axial_attn_fwd")
        return out

    @torch.no_grad()
    def block(self, x: Tensor, stage: int, index: int) -> Tensor:
        """SingleBlock `index` of `stage`: x [N, cin, h, w] -> [N, 4 b, h, w]"""
        self._require_eval()
        x = _dev_f32(x, "x")
        b, cin = self._dec_channels[stage], kmax_pix_block_cin(self._in_channels[0], self._dec_channels, stage, index)
        if x.dim() != 4 or x.shape[1] != cin:
            raise RuntimeError(f"axial_vs_amd: x {tuple(x.shape)} must be [N, {cin}, h, w]")
        N, _, h, w = x.shape
        with _on(x.device):
            cfg = self._stage_cfg({stage: (h, w)}, N)
            st = _stream(x.device)
            ws = _workspace_for("axvs_kmax_pix_workspace_bytes", x.device, st, C.byref(cfg))
            out = torch.empty(N, 4 * b, h, w, dtype=torch.float32, device=x.device)
            _lib.check(_lib.lib().axvs_kmax_pix_block_fwd(C.byref(cfg), self._packed().data_ptr(), self._locate(stage, index), x.data_ptr(), out.data_ptr(),
                                                          ws.data_ptr(), ws.numel(), st), "axvs_kmax_pix_block_fwd")
        return out

    @torch.no_grad()
    def fuse(self, low: Tensor, high: Tensor, index: int) -> Tensor:
        """ResizedFuse `index` (in front of stage index + 1) with the LayerNorm of its high-resolution input: low [N, 4 b_prev, hl, wl] (a
        stage's raw output), high [N, in_channels[index + 1], h, w] (the backbone feature) -> [N, b, h, w]"""
        self._require_eval()
        low, high = _dev_f32(low, "low"), _dev_f32(high, "high")
        i = index + 1
        if not 0 <= index < 3 or low.dim() != 4 or high.dim() != 4 or low.shape[1] != 4 * self._dec_channels[i - 1] or high.shape[1] != self._in_channels[i] \
                or low.shape[0] != high.shape[0]:
            raise RuntimeError(f"axial_vs_amd: low {tuple(low.shape)}, high {tuple(high.shape)} must be [N, {4 * self._dec_channels[i - 1]}, hl, wl], "
                               f"[N, {self._in_channels[i]}, h, w]")
        N = low.shape[0]
        with _on(low.device):
            cfg = self._stage_cfg({i - 1: tuple(low.shape[-2:]), i: tuple(high.shape[-2:])}, N)
            st = _stream(low.device)
            ws = _workspace_for("axvs_kmax_pix_workspace_bytes", low.device, st, C.byref(cfg))
            out = torch.empty(N, self._dec_channels[i], *high.shape[-2:], dtype=torch.float32, device=low.device)
            _lib.check(_lib.lib().axvs_kmax_pix_fuse_fwd(C.byref(cfg), self._packed().data_ptr(), index, low.data_ptr(), high.data_ptr(), out.data_ptr(),
                                                         ws.data_ptr(), ws.numel(), st), "axvs_kmax_pix_fuse_fwd")
        return out


class MaXTronDeepLabHead(nn.Module):
    """`MaXTronDeepLabHead` under the reference's child names (`wc_module`, `pixel_decoder`, `predictor`): a checkpoint's `sem_seg_head.*`
    state loads into it.  `layers(features)` / `forward(features)`: the within-clip module (when there is one), the pixel decoder, the
    query decoder -> the predictor's dict, bit-equal to calling the three by hand."""

    def __init__(self, wc_module, pixel_decoder: nn.Module, predictor: nn.Module):
        super().__init__()
        self.wc_module = wc_module
        self.pixel_decoder = pixel_decoder
        self.predictor = predictor

    def forward(self, features):
        return self.layers(features)

    def layers(self, features):
        if self.wc_module is not None:
            features, _, _ = self.wc_module.forward_features(features)
        panoptic_features, semantic_features, multi_scale_features = self.pixel_decoder.forward_features(features)
        return self.predictor(multi_scale_features, panoptic_features, semantic_features)
