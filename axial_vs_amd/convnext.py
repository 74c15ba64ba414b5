"""The ConvNeXt / ConvNeXtV2 backbone on the device (eval-mode forward).

Reference (MaXTron_Video-kMaX): `ConvNeXt` / `D2ConvNeXt` (kmax_deeplab/modeling/backbone/convnext.py:15-216) and `ConvNeXtV2` /
`D2ConvNeXtV2` (convnextv2.py:15-214), under their own state-dict names.

Activations travel channels-last (rows [N][h][w][C], fp32) from the stem to the last block; only the requested outputs are written as
NCHW.  The patchify convolutions are a gather kernel (the reference's zero padding comes from its index test; in front of a downsample
layer the padding is applied BEFORE the LayerNorm, so a padded pixel carries the LayerNorm's bias) and one split-precision GEMM.  A
block is one fused depthwise 7x7 + LayerNorm kernel, pwconv1 + gelu as one GEMM, pwconv2 + residual as one GEMM (V1: the layer scale
folded into it; V2: one GEMM per frame on W2 diag(s_n), s_n from the frame's own GRN statistics).  Frames are independent.

Forward only: `train()` mode raises NotImplementedError at `forward` (DropPath and training are not part of the device path).
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Dict, Mapping, Sequence

import torch
import torch.nn as nn
from torch import Tensor

from . import _lib
from ._params import convnext_block_folded, convnext_down_folded
from .modules import _cached_pack, _dev_f32, _on, _pack_folded, _stream, _workspace_for

ShapeSpec = namedtuple("ShapeSpec", ["channels", "stride"])       # what `output_shape()` holds: the two fields the pixel decoders read

_NAMES = ("stem", "res2", "res3", "res4", "res5")
_STRIDES = {"stem": 2, "res2": 4, "res3": 8, "res4": 16, "res5": 32}      # (the reference's own table: it lists the stem at 2)
_MAX_DIM, _MAX_DEPTH = 2048, 64


def map_sizes(H: int, W: int):
    """the four stages' map sizes for an image of H x W: floor((H + 3) / 4), then floor((h + 1) / 2) per stage"""
    h, w = (int(H) + 3) // 4, (int(W) + 3) // 4
    out = []
    for _ in range(4):
        out.append((h, w))
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


def _check_config(in_chans, depths, dims) -> None:
    if int(in_chans) != 3:
        raise NotImplementedError(f"axial_vs_amd: the ConvNeXt stem kernel takes in_chans = 3 (got {in_chans})")
    if len(depths) != 4 or len(dims) != 4:
        raise NotImplementedError(f"axial_vs_amd: the ConvNeXt kernels take four stages (got depths {list(depths)}, dims {list(dims)})")
    for d in dims:
        if int(d) % 16 or not 16 <= int(d) <= _MAX_DIM:
            raise NotImplementedError(f"axial_vs_amd: dims {list(dims)} must be multiples of 16 in 16..{_MAX_DIM}")
    for n in depths:
        if not 1 <= int(n) <= _MAX_DEPTH:
            raise NotImplementedError(f"axial_vs_amd: the ConvNeXt kernels take 1..{_MAX_DEPTH} blocks per stage (depths {list(depths)})")


def _cfg(N: int, H: int, W: int, sizes, depths, dims, v2: bool) -> _lib.AxvsCnxCfg:
    i4 = C.c_int * 4
    return _lib.AxvsCnxCfg(N=int(N), H=int(H), W=int(W), dims=i4(*[int(d) for d in dims]), depths=i4(*[int(n) for n in depths]),
                           h=i4(*[int(s[0]) for s in sizes]), w=i4(*[int(s[1]) for s in sizes]), v2=int(bool(v2)))


def _pack(sd: Mapping[str, Tensor], depths, dims, v2: bool) -> Tensor:
    """fold (float64) and pack: one blob of fp32 tensors in the kernels' layouts"""
    sd = {k: v.detach() for k, v in sd.items()}
    downs = (convnext_down_folded(sd, i) for i in range(4))
    blocks = (convnext_block_folded(sd, f"stages.{i}.{j}.") for i in range(4) for j in range(int(depths[i])))
    return _pack_folded("axvs_cnx", _cfg(1, 1, 1, [(1, 1)] * 4, depths, dims, v2), [(_lib.AxvsCnxDownParams, downs), (_lib.AxvsCnxBlockParams, blocks)])


def _image(x: Tensor) -> Tensor:
    if x.dim() != 4 or x.shape[1] != 3:
        raise RuntimeError(f"axial_vs_amd: ConvNeXt takes an input of shape (N, 3, H, W), got {tuple(x.shape)}")
    return _dev_f32(x, "x")        # (a channels_last image is copied to NCHW here: the same numbers, so the same bits)


def _run(packed: Tensor, x: Tensor, depths, dims, v2: bool, want: Sequence[str]) -> Dict[str, Tensor]:
    N, _, H, W = x.shape
    sizes = map_sizes(H, W)
    dev = x.device
    cfg = _cfg(N, H, W, sizes, depths, dims, v2)
    st = _stream(dev)
    ws = _workspace_for("axvs_cnx_workspace_bytes", dev, st, C.byref(cfg))
    shape = {"stem": (dims[0], sizes[0])}
    shape.update({f"res{i + 2}": (dims[i], sizes[i]) for i in range(4)})
    outs = {k: torch.empty(N, int(shape[k][0]), *shape[k][1], dtype=torch.float32, device=dev) for k in _NAMES if k in want}
    op = (C.c_void_p * 5)(*[outs[k].data_ptr() if k in outs else None for k in _NAMES])
    _lib.check(_lib.lib().axvs_cnx_fwd(C.byref(cfg), packed.data_ptr(), x.data_ptr(), op, ws.data_ptr(), ws.numel(), st), "axvs_cnx_fwd")
    return outs


def _depths_of(params: Mapping[str, Tensor]):
    return [1 + max(int(k.split(".")[2]) for k in params if k.startswith(f"stages.{i}.")) for i in range(4)]


@torch.no_grad()
def convnext_forward(params: Mapping[str, Tensor], x: Tensor, out_features: Sequence[str] = ("res2", "res3", "res4", "res5")) -> Dict[str, Tensor]:
    """The backbone's eval forward from a mapping of the reference's state-dict names to GPU tensors: ConvNeXtV2 when the mapping has
    `stages.0.0.grn.gamma`, else ConvNeXt (with or without `gamma`).  Folds and packs the parameters on every call: the modules keep the
    packed weights.  -> {name: [N, C, h, w]} for the names of `out_features` out of stem, res2 .. res5."""
    depths = _depths_of(params)
    dims = [int(params[f"downsample_layers.{i}.{0 if i == 0 else 1}.weight"].shape[0]) for i in range(4)]
    _check_config(params["downsample_layers.0.0.weight"].shape[1], depths, dims)
    v2 = "stages.0.0.grn.gamma" in params
    x = _image(x)
    with _on(x.device):
        return _run(_pack(params, depths, dims, v2), x, depths, dims, v2, tuple(out_features))


class _LayerNorm(nn.Module):
    """the state of the reference's LayerNorm (eps 1e-6), either data format"""

    def __init__(self, channels: int):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(channels))
        self.bias = nn.Parameter(torch.zeros(channels))


class _GRN(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.gamma = nn.Parameter(torch.zeros(1, 1, 1, dim))
        self.beta = nn.Parameter(torch.zeros(1, 1, 1, dim))


class _Block(nn.Module):
    def __init__(self, dim: int, v2: bool, layer_scale_init_value: float):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim)
        self.norm = _LayerNorm(dim)
        self.pwconv1 = nn.Linear(dim, 4 * dim)
        if v2:
            self.grn = _GRN(4 * dim)
        self.pwconv2 = nn.Linear(4 * dim, dim)
        if not v2 and layer_scale_init_value > 0:
            self.gamma = nn.Parameter(layer_scale_init_value * torch.ones(dim))


class _Backbone(nn.Module):
    _v2 = False

    def __init__(self, in_chans, depths, dims, drop_path_rate, layer_scale_init_value, out_indices, out_features):
        super().__init__()
        _check_config(in_chans, depths, dims)
        self._depths, self._dims = [int(n) for n in depths], [int(d) for d in dims]
        self.num_features = list(self._dims)
        self.drop_path_rate = float(drop_path_rate)          # (training only: the device path is the eval forward)
        self.out_indices = [int(i) for i in out_indices]
        self._out_features = [str(k) for k in out_features]
        for k in self._out_features:
            if k not in _NAMES:
                raise ValueError(f"axial_vs_amd: out_features {list(out_features)} must be out of {list(_NAMES)}")
        self._out_feature_strides = dict(_STRIDES)
        self._out_feature_channels = {"stem": self._dims[0], **{f"res{i + 2}": self._dims[i] for i in range(4)}}
        d = self._dims
        self.downsample_layers = nn.ModuleList([nn.Sequential(nn.Conv2d(3, d[0], kernel_size=4, stride=4), _LayerNorm(d[0]))]
                                               + [nn.Sequential(_LayerNorm(d[i]), nn.Conv2d(d[i], d[i + 1], kernel_size=2, stride=2)) for i in range(3)])
        self.stages = nn.ModuleList([nn.Sequential(*[_Block(d[i], self._v2, layer_scale_init_value) for _ in range(self._depths[i])]) for i in range(4)])

    def _packed(self) -> Tensor:
        return _cached_pack(self, "cnx", "f32", (self,), lambda dt: _pack(dict(self.named_parameters()), self._depths, self._dims, self._v2))

    def _require_eval(self) -> None:
        if self.training:
            raise NotImplementedError(f"axial_vs_amd: {type(self).__name__} has a forward-only HIP path -- call .eval() (DropPath and "
                                      "training are not part of it)")

    def _names(self):
        """what the reference's forward returns: the stem and the stages of out_indices, filtered by out_features"""
        made = ["stem"] + [f"res{i + 2}" for i in range(4) if i in self.out_indices]
        return [k for k in made if k in self._out_features]

    @torch.no_grad()
    def forward(self, x: Tensor) -> Dict[str, Tensor]:
        self._require_eval()
        x = _image(x)
        with _on(x.device):
            return _run(self._packed(), x, self._depths, self._dims, self._v2, self._names())

    def output_shape(self):
        return {name: ShapeSpec(channels=self._out_feature_channels[name], stride=self._out_feature_strides[name]) for name in self._out_features}

    @property
    def size_divisibility(self):
        return -1

    # ---- step entries (what the tests read): channels-last rows in and out, any map size inside the kernels' bounds ----------------------
    def _locate(self, stage: int, index: int) -> int:
        if not (0 <= stage < 4 and 0 <= index < self._depths[stage]):
            raise IndexError(f"axial_vs_amd: stage {stage} has no block {index}")
        return sum(self._depths[:stage]) + index

    def _step(self, x: Tensor, stage: int, what: str):
        self._require_eval()
        x = _dev_f32(x, "x")
        if x.dim() != 4 or x.shape[3] != self._dims[stage]:
            raise RuntimeError(f"axial_vs_amd: {what}: x {tuple(x.shape)} must be [N, h, w, {self._dims[stage]}]")
        return x

    @torch.no_grad()
    def stem(self, x: Tensor) -> Tensor:
        """`downsample_layers.0` behind the reference's padding: x [N, 3, H, W] -> [N, h, w, dims[0]] (channels-last)"""
        self._require_eval()
        x = _image(x)
        N, _, H, W = x.shape
        sizes = map_sizes(H, W)
        with _on(x.device):
            cfg = _cfg(N, H, W, sizes, self._depths, self._dims, self._v2)
            st = _stream(x.device)
            ws = _workspace_for("axvs_cnx_workspace_bytes", x.device, st, C.byref(cfg))
            out = torch.empty(N, *sizes[0], self._dims[0], dtype=torch.float32, device=x.device)
            _lib.check(_lib.lib().axvs_cnx_stem_fwd(C.byref(cfg), self._packed().data_ptr(), x.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), st),
                       "axvs_cnx_stem_fwd")
        return out

    @torch.no_grad()
    def downsample(self, x: Tensor, index: int) -> Tensor:
        """`downsample_layers.{index}` (1..3) behind the reference's padding: x [N, h, w, dims[index - 1]] -> [N, (h+1)//2, (w+1)//2, dims[index]]"""
        if not 1 <= index <= 3:
            raise IndexError(f"axial_vs_amd: downsample layer {index} is not one of 1..3")
        x = self._step(x, index - 1, "downsample")
        N, h, w, _ = x.shape
        sizes = [(1, 1)] * 4
        sizes[index - 1], sizes[index] = (h, w), ((h + 1) // 2, (w + 1) // 2)
        with _on(x.device):
            cfg = _cfg(N, 1, 1, sizes, self._depths, self._dims, self._v2)
            st = _stream(x.device)
            ws = _workspace_for("axvs_cnx_workspace_bytes", x.device, st, C.byref(cfg))
            out = torch.empty(N, *sizes[index], self._dims[index], dtype=torch.float32, device=x.device)
            _lib.check(_lib.lib().axvs_cnx_down_fwd(C.byref(cfg), self._packed().data_ptr(), index, x.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), st),
                       "axvs_cnx_down_fwd")
        return out

    def _block_call(self, x: Tensor, stage: int, index: int, whole: bool) -> Tensor:
        x = self._step(x, stage, "block")
        N, h, w, _ = x.shape
        sizes = [(1, 1)] * 4
        sizes[stage] = (h, w)
        with _on(x.device):
            cfg = _cfg(N, 1, 1, sizes, self._depths, self._dims, self._v2)
            st = _stream(x.device)
            out = torch.empty_like(x)
            if whole:
                ws = _workspace_for("axvs_cnx_workspace_bytes", x.device, st, C.byref(cfg))
                _lib.check(_lib.lib().axvs_cnx_block_fwd(C.byref(cfg), self._packed().data_ptr(), self._locate(stage, index), x.data_ptr(), out.data_ptr(),
                                                         ws.data_ptr(), ws.numel(), st), "axvs_cnx_block_fwd")
            else:
                _lib.check(_lib.lib().axvs_cnx_dwln_fwd(C.byref(cfg), self._packed().data_ptr(), self._locate(stage, index), x.data_ptr(), out.data_ptr(), st),
                           "axvs_cnx_dwln_fwd")
        return out

    @torch.no_grad()
    def dwconv_norm(self, x: Tensor, stage: int, index: int) -> Tensor:
        """the depthwise 7x7 and the LayerNorm of block `index` of `stage`: x [N, h, w, C] -> [N, h, w, C]"""
        return self._block_call(x, stage, index, False)

    @torch.no_grad()
    def block(self, x: Tensor, stage: int, index: int) -> Tensor:
        """block `index` of `stage`: x [N, h, w, C] -> [N, h, w, C]"""
        return self._block_call(x, stage, index, True)


class ConvNeXtBackbone(_Backbone):
    """`ConvNeXt` / `D2ConvNeXt` under the reference's own parameter names: a checkpoint's `backbone.*` state loads with
    `load_state_dict(strict=True)`.  forward(x [N, 3, H, W]) -> {name: [N, C, h, w] fp32} for the names of `out_features` among the stem and
    the stages of `out_indices`; the dict feeds `KMaXPixelDecoder.forward_features` / `MaXTronDeepLabHead` as it is.  GPU tensors only; eval()
    only; runs on the current stream; the folded weights are packed once and again when a parameter changes (`invalidate_pack` forgets
    them).  Bounds (NotImplementedError at construction): in_chans 3; four stages of 1..64 blocks; dims multiples of 16 in 16..2048.
    `layer_scale_init_value <= 0`: blocks without `gamma`."""

    def __init__(self, in_chans: int = 3, depths: Sequence[int] = (3, 3, 27, 3), dims: Sequence[int] = (192, 384, 768, 1536), drop_path_rate: float = 0.,
                 layer_scale_init_value: float = 1e-6, out_indices: Sequence[int] = (0, 1, 2, 3),
                 out_features: Sequence[str] = ("res2", "res3", "res4", "res5")):
        super().__init__(in_chans, depths, dims, drop_path_rate, float(layer_scale_init_value), out_indices, out_features)


class ConvNeXtV2Backbone(_Backbone):
    """`ConvNeXtV2` / `D2ConvNeXtV2`: as `ConvNeXtBackbone`, with Global Response Normalization (`grn.gamma`, `grn.beta` of shape
    [1, 1, 1, 4 dim]) in place of the layer scale.  A frame's GRN statistics are its own."""
    _v2 = True

    def __init__(self, in_chans: int = 3, depths: Sequence[int] = (3, 3, 27, 3), dims: Sequence[int] = (192, 384, 768, 1536), drop_path_rate: float = 0.,
                 out_indices: Sequence[int] = (0, 1, 2, 3), out_features: Sequence[str] = ("res2", "res3", "res4", "res5")):
        super().__init__(in_chans, depths, dims, drop_path_rate, 0.0, out_indices, out_features)
