"""The ResNet bottleneck backbone on the device (eval-mode forward).

Reference (MaXTron_Video-kMaX): `BasicStem`, `BottleneckBlock`, `ResNet` and `custom_bn_build_resnet_backbone`
(kmax_deeplab/modeling/backbone/resnet.py:103-214, 333-493, 616-697), under their own state-dict names.

Activations travel channels-last (rows [N][h][w][C], fp32) from the stem's output to the last block; only the requested outputs are
written as NCHW.  Every BatchNorm is folded in float64 at pack time (running statistics, the module's eps) into its convolution.  The stem
(7x7 / stride 2 convolution, ReLU, 3x3 / stride 2 max pool) is one kernel; a block is conv1 as one split-precision GEMM, the 3x3 as one
implicit-GEMM kernel on the same three-piece products, the projection shortcut as one GEMM and conv3 as one GEMM that ends in
relu(... + shortcut); a stride-2 1x1 convolution reads rows picked by a gather kernel.  Frames are independent.

Forward only: `train()` mode raises NotImplementedError at `forward` (BatchNorm on batch statistics is not part of the device path).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Mapping, Optional, Sequence

import torch
import torch.nn as nn
from torch import Tensor

from . import _lib
from ._params import resnet_block_folded, resnet_stem_folded
from .convnext import ShapeSpec
from .modules import _cached_pack, _dev_f32, _on, _pack_folded, _stream, _workspace_for

_NAMES = ("stem", "res2", "res3", "res4", "res5")
_BLOCKS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}
_BN_EPS = 1e-3          # the reference's get_norm("SyncBN", .)


def _ceil_half(x: int) -> int:
    return (int(x) + 1) // 2


class _Config:
    """what the kernels need to know of a network: channels, blocks, strides, dilations"""

    def __init__(self, in_channels, stem, widths, outs, blocks, stride_in_1x1, res5_dilation):
        if res5_dilation not in (1, 2):
            raise NotImplementedError(f"axial_vs_amd: res5_dilation {res5_dilation} is not built (the reference takes 1 or 2)")
        self.in_channels, self.stem = int(in_channels), int(stem)
        self.widths, self.outs, self.blocks = [int(v) for v in widths], [int(v) for v in outs], [int(v) for v in blocks]
        self.stride_in_1x1 = bool(stride_in_1x1)
        self.strides = [1, 2, 2, 1 if res5_dilation == 2 else 2]
        self.dilations = [1, 1, 1, int(res5_dilation)]
        if self.in_channels != 3:
            raise NotImplementedError(f"axial_vs_amd: the ResNet stem kernel takes 3-channel images (got {in_channels})")
        if len(self.blocks) != 4:
            raise NotImplementedError(f"axial_vs_amd: the ResNet kernels take four stages (got blocks {list(blocks)})")
        if self.stem % 16 or not 16 <= self.stem <= 128:
            raise NotImplementedError(f"axial_vs_amd: stem_out_channels {stem} must be a multiple of 16 in 16..128")
        for n in self.blocks:
            if not 1 <= n <= 64:
                raise NotImplementedError(f"axial_vs_amd: the ResNet kernels take 1..64 blocks per stage (got {list(blocks)})")
        for v in self.widths:
            if v % 32 or not 32 <= v <= 512:
                raise NotImplementedError(f"axial_vs_amd: bottleneck widths {self.widths} must be multiples of 32 in 32..512")
        for v in self.outs:
            if v % 16 or not 16 <= v <= 2048:
                raise NotImplementedError(f"axial_vs_amd: stage output channels {self.outs} must be multiples of 16 in 16..2048")

    def in_of(self, stage: int) -> int:
        return self.stem if stage == 0 else self.outs[stage - 1]

    def stage_sizes(self, H: int, W: int):
        """the maps the four stages READ for an image of H x W"""
        h, w = _ceil_half(_ceil_half(H)), _ceil_half(_ceil_half(W))
        sizes = []
        for s in self.strides:
            sizes.append((h, w))
            h, w = -(-h // s), -(-w // s)
        return sizes

    def out_size(self, stage: int, size):
        s = self.strides[stage]
        return (-(-size[0] // s), -(-size[1] // s))

    def cfg(self, N: int, H: int, W: int, sizes) -> _lib.AxvsRnCfg:
        i4 = C.c_int * 4
        return _lib.AxvsRnCfg(N=int(N), H=int(H), W=int(W), in_channels=self.in_channels, stem_channels=self.stem, width=i4(*self.widths),
                              out_channels=i4(*self.outs), blocks=i4(*self.blocks), stride=i4(*self.strides), dilation=i4(*self.dilations),
                              h=i4(*[int(s[0]) for s in sizes]), w=i4(*[int(s[1]) for s in sizes]), stride_in_1x1=int(self.stride_in_1x1))

    def pack(self, sd: Mapping[str, Tensor], eps: float) -> Tensor:
        """fold (float64) and pack: one blob of fp32 tensors and split 3x3 weights in the kernels' layouts"""
        sd = {k: v.detach() for k, v in sd.items()}
        blocks = (resnet_block_folded(sd, f"res{i + 2}.{j}.", eps) for i in range(4) for j in range(self.blocks[i]))
        return _pack_folded("axvs_rn", self.cfg(1, 1, 1, [(1, 1)] * 4), [(_lib.AxvsRnStemParams, [resnet_stem_folded(sd, eps)]), (_lib.AxvsRnBlockParams, blocks)])

    def run(self, packed: Tensor, x: Tensor, want: Sequence[str]) -> Dict[str, Tensor]:
        N, _, H, W = x.shape
        sizes = self.stage_sizes(H, W)
        dev = x.device
        cfg = self.cfg(N, H, W, sizes)
        st = _stream(dev)
        ws = _workspace_for("axvs_rn_workspace_bytes", dev, st, C.byref(cfg))
        shape = {"stem": (self.stem, sizes[0])}
        shape.update({f"res{i + 2}": (self.outs[i], self.out_size(i, sizes[i])) for i in range(4)})
        outs = {k: torch.empty(N, int(shape[k][0]), *shape[k][1], dtype=torch.float32, device=dev) for k in want}
        op = (C.c_void_p * 5)(*[outs[k].data_ptr() if k in outs else None for k in _NAMES])
        _lib.check(_lib.lib().axvs_rn_fwd(C.byref(cfg), packed.data_ptr(), x.data_ptr(), op, st, ws.data_ptr(), ws.numel()), "axvs_rn_fwd")
        return outs


def _image(x: Tensor) -> Tensor:
    if x.dim() != 4 or x.shape[1] != 3:
        raise RuntimeError(f"axial_vs_amd: ResNet takes an input of shape (N, 3, H, W), got {tuple(x.shape)}")
    return _dev_f32(x, "x")        # (a channels_last image is copied to NCHW here: the same numbers, so the same bits)


def _check_names(out_features) -> list:
    names = [str(k) for k in out_features]
    for k in names:
        if k not in _NAMES:
            raise ValueError(f"axial_vs_amd: out_features {list(out_features)} must be out of {list(_NAMES)}")
    return names


@torch.no_grad()
def resnet_forward(params: Mapping[str, Tensor], x: Tensor, out_features: Sequence[str] = ("res2", "res3", "res4", "res5"), *,
                   stride_in_1x1: bool = False, res5_dilation: int = 1, eps: float = _BN_EPS) -> Dict[str, Tensor]:
    """The backbone's eval forward from a mapping of the reference's state-dict names to GPU tensors.  Depths and widths are read off the
    shapes; where the stride sits and res5's dilation are not in a state dict, so they are keyword arguments.  Folds and packs the parameters
    on every call: the module keeps the packed weights.  -> {name: [N, C, h, w]} in `out_features` order, names out of stem, res2 .. res5."""
    blocks = [1 + max(int(k.split(".")[1]) for k in params if k.startswith(f"res{i + 2}.")) for i in range(4)]
    conf = _Config(params["stem.conv1.weight"].shape[1], params["stem.conv1.weight"].shape[0], [params[f"res{i + 2}.0.conv2.weight"].shape[0] for i in range(4)],
                   [params[f"res{i + 2}.0.conv3.weight"].shape[0] for i in range(4)], blocks, stride_in_1x1, res5_dilation)
    if params["res2.0.conv2.weight"].shape[1] != params["res2.0.conv2.weight"].shape[0]:
        raise NotImplementedError("axial_vs_amd: grouped 3x3 convolutions (ResNeXt) are not built")
    names = _check_names(out_features)
    x = _image(x)
    with _on(x.device):
        return conf.run(conf.pack(params, eps), x, names)


class _ConvBN(nn.Conv2d):
    """the state of detectron2's `Conv2d(..., bias=False, norm=BatchNorm)`: `weight` and `norm.*`"""

    def __init__(self, cin: int, cout: int, kernel_size: int, eps: float, **kw):
        super().__init__(cin, cout, kernel_size, bias=False, **kw)
        self.norm = nn.BatchNorm2d(cout, eps=eps, momentum=0.01)


class _Stem(nn.Module):
    def __init__(self, cin: int, cout: int, eps: float):
        super().__init__()
        self.conv1 = _ConvBN(cin, cout, 7, eps, stride=2, padding=3)


class _Bottleneck(nn.Module):
    def __init__(self, cin: int, cout: int, width: int, stride: int, stride_in_1x1: bool, dilation: int, eps: float):
        super().__init__()
        if cin != cout:
            self.shortcut = _ConvBN(cin, cout, 1, eps, stride=stride)
        else:
            self.shortcut = None
        s1, s3 = (stride, 1) if stride_in_1x1 else (1, stride)
        self.conv1 = _ConvBN(cin, width, 1, eps, stride=s1)
        self.conv2 = _ConvBN(width, width, 3, eps, stride=s3, padding=dilation, dilation=dilation)
        self.conv3 = _ConvBN(width, cout, 1, eps)


class ResNetBackbone(nn.Module):
    """`custom_bn_build_resnet_backbone`'s ResNet (bottleneck depths 50 / 101 / 152, or `num_blocks`) under the reference's own parameter
    names: a checkpoint's `backbone.*` state loads with `load_state_dict(strict=True)`.  forward(x [N, 3, H, W]) -> {name: [N, C, h, w] fp32}
    in `out_features` order; the dict feeds `KMaXPixelDecoder.forward_features` / `WithinClipTrackingModule.forward_features` /
    `MaXTronDeepLabHead` as it is.  GPU tensors only; eval() only; runs on the current stream; the folded weights are packed once and again
    when a parameter or a running statistic changes (`invalidate_pack` forgets them).  All four stages are always built (the reference drops
    the stages behind the last requested one).  Not built (NotImplementedError at construction): depths 18 / 34 (BasicBlock), num_groups > 1
    (ResNeXt), deformable stages, res5_dilation outside {1, 2}, a norm other than "SyncBN" / "BN"; bounds: 3-channel images, 1..64 blocks per
    stage, bottleneck widths multiples of 32 in 32..512, stem width a multiple of 16 in 16..128, stage outputs multiples of 16 up to 2048.
    `bottleneck_channels` / `stage_out_channels` (four values each) replace the builder's doubling rule, as `ResNet.make_stage` allows."""

    def __init__(self, depth: Optional[int] = 50, num_blocks: Optional[Sequence[int]] = None, stem_out_channels: int = 64, res2_out_channels: int = 256,
                 num_groups: int = 1, width_per_group: int = 64, stride_in_1x1: bool = False, res5_dilation: int = 1, norm: str = "SyncBN",
                 out_features: Sequence[str] = ("res2", "res3", "res4", "res5"), in_channels: int = 3, deform_on_per_stage: Sequence[bool] = (False,) * 4,
                 bottleneck_channels: Optional[Sequence[int]] = None, stage_out_channels: Optional[Sequence[int]] = None):
        super().__init__()
        if num_blocks is None:
            if depth in (18, 34):
                raise NotImplementedError(f"axial_vs_amd: ResNet-{depth} is made of BasicBlocks, which are not built (bottleneck depths: {sorted(_BLOCKS)})")
            if depth not in _BLOCKS:
                raise NotImplementedError(f"axial_vs_amd: ResNet depth {depth} is not one of {sorted(_BLOCKS)}; pass num_blocks for another bottleneck network")
            num_blocks = _BLOCKS[depth]
        if int(num_groups) != 1:
            raise NotImplementedError(f"axial_vs_amd: num_groups = {num_groups}: grouped 3x3 convolutions (ResNeXt) are not built")
        if any(deform_on_per_stage):
            raise NotImplementedError("axial_vs_amd: deformable bottleneck stages are not built")
        if str(norm).lower() not in ("syncbn", "bn"):
            raise NotImplementedError(f"axial_vs_amd: norm {norm!r} is not built: the device path folds an eval BatchNorm (\"SyncBN\" / \"BN\")")
        eps = _BN_EPS if str(norm).lower() == "syncbn" else 1e-5
        width = int(num_groups) * int(width_per_group)
        # (the builder's rule: both double from stage to stage; `ResNet.make_stage` takes any, so the two sequences may state them per stage)
        widths = [width << i for i in range(4)] if bottleneck_channels is None else list(bottleneck_channels)
        outs = [int(res2_out_channels) << i for i in range(4)] if stage_out_channels is None else list(stage_out_channels)
        if len(widths) != 4 or len(outs) != 4:
            raise NotImplementedError(f"axial_vs_amd: the ResNet kernels take four stages (got widths {widths}, outputs {outs})")
        self._conf = _Config(in_channels, stem_out_channels, widths, outs, num_blocks, stride_in_1x1, res5_dilation)
        self._out_features = _check_names(out_features)
        conf = self._conf
        self.stem = _Stem(conf.in_channels, conf.stem, eps)
        self._out_feature_strides, self._out_feature_channels = {"stem": 4}, {"stem": conf.stem}
        stride = 4
        for i in range(4):
            blocks = [_Bottleneck(conf.in_of(i) if j == 0 else conf.outs[i], conf.outs[i], conf.widths[i], conf.strides[i] if j == 0 else 1, conf.stride_in_1x1,
                                  conf.dilations[i], eps) for j in range(conf.blocks[i])]
            setattr(self, f"res{i + 2}", nn.Sequential(*blocks))
            stride *= conf.strides[i]
            self._out_feature_strides[f"res{i + 2}"], self._out_feature_channels[f"res{i + 2}"] = stride, conf.outs[i]

    def _eps(self) -> float:
        return float(self.stem.conv1.norm.eps)

    def _packed(self) -> Tensor:
        return _cached_pack(self, "rn", "f32", (self,), lambda dt: self._conf.pack(self.state_dict(), self._eps()), buffers=True)

    def _require_eval(self) -> None:
        if self.training:
            raise NotImplementedError("axial_vs_amd: ResNetBackbone has a forward-only HIP path -- call .eval() (BatchNorm on batch statistics and "
                                      "training are not part of it)")

    @torch.no_grad()
    def forward(self, x: Tensor) -> Dict[str, Tensor]:
        self._require_eval()
        x = _image(x)
        with _on(x.device):
            outs = self._conf.run(self._packed(), x, self._out_features)
        return {k: outs[k] for k in self._out_features}

    def output_shape(self):
        return {name: ShapeSpec(channels=self._out_feature_channels[name], stride=self._out_feature_strides[name]) for name in self._out_features}

    @property
    def size_divisibility(self):
        return 0

    # ---- step entries (what the tests read): channels-last rows in and out, any map size inside the kernels' bounds ----------------------
    def _locate(self, stage: int, index: int) -> int:
        if not (0 <= stage < 4 and 0 <= index < self._conf.blocks[stage]):
            raise IndexError(f"axial_vs_amd: stage {stage} has no block {index}")
        return sum(self._conf.blocks[:stage]) + index

    @torch.no_grad()
    def stem_rows(self, x: Tensor) -> Tensor:
        """the stem: x [N, 3, H, W] -> [N, h, w, stem_out_channels] (channels-last)"""
        self._require_eval()
        x = _image(x)
        N, _, H, W = x.shape
        conf = self._conf
        sizes = [conf.stage_sizes(H, W)[0]] + [(1, 1)] * 3
        with _on(x.device):
            cfg = conf.cfg(N, H, W, sizes)
            out = torch.empty(N, *sizes[0], conf.stem, dtype=torch.float32, device=x.device)
            _lib.check(_lib.lib().axvs_rn_stem_fwd(C.byref(cfg), self._packed().data_ptr(), x.data_ptr(), out.data_ptr(), _stream(x.device)), "axvs_rn_stem_fwd")
        return out

    def _step_cfg(self, x: Tensor, stage: int, index: int, channels: int, what: str, read_scale: int):
        """the configuration in which block `index` of `stage` reads x's map (a later block reads the map the stage leaves: the stage's
        own input map is `read_scale` times as large)"""
        self._require_eval()
        x = _dev_f32(x, "x")
        if x.dim() != 4 or x.shape[3] != channels:
            raise RuntimeError(f"axial_vs_amd: {what}: x {tuple(x.shape)} must be [N, h, w, {channels}]")
        N, h, w, _ = x.shape
        sizes = [(1, 1)] * 4
        sizes[stage] = (h * read_scale, w * read_scale)
        return x, self._conf.cfg(N, 1, 1, sizes)

    @torch.no_grad()
    def conv3x3(self, x: Tensor, stage: int, index: int) -> Tensor:
        """`conv2` + BatchNorm + ReLU of block `index` of `stage` on conv1's map: x [N, h, w, width] -> [N, ceil(h / s), ceil(w / s), width]"""
        conf = self._conf
        at = self._locate(stage, index)
        first = index == 0
        s3 = conf.strides[stage] if first and not conf.stride_in_1x1 else 1
        # conv1's map is the block's input map unless the stride sits in conv1; a later block reads the map the stage leaves
        scale = conf.strides[stage] if (not first or conf.stride_in_1x1) else 1
        x, cfg = self._step_cfg(x, stage, index, conf.widths[stage], "conv3x3", scale)
        N, h, w, _ = x.shape
        with _on(x.device):
            out = torch.empty(N, -(-h // s3), -(-w // s3), conf.widths[stage], dtype=torch.float32, device=x.device)
            _lib.check(_lib.lib().axvs_rn_conv3_fwd(C.byref(cfg), self._packed().data_ptr(), at, x.data_ptr(), out.data_ptr(), _stream(x.device)), "axvs_rn_conv3_fwd")
        return out

    @torch.no_grad()
    def block(self, x: Tensor, stage: int, index: int) -> Tensor:
        """block `index` of `stage`: x [N, h, w, in] -> [N, ceil(h / s), ceil(w / s), out], s the block's stride"""
        conf = self._conf
        at = self._locate(stage, index)
        first = index == 0
        s = conf.strides[stage] if first else 1
        x, cfg = self._step_cfg(x, stage, index, conf.in_of(stage) if first else conf.outs[stage], "block", 1 if first else conf.strides[stage])
        N, h, w, _ = x.shape
        with _on(x.device):
            st = _stream(x.device)
            ws = _workspace_for("axvs_rn_workspace_bytes", x.device, st, C.byref(cfg))
            out = torch.empty(N, -(-h // s), -(-w // s), conf.outs[stage], dtype=torch.float32, device=x.device)
            _lib.check(_lib.lib().axvs_rn_block_fwd(C.byref(cfg), self._packed().data_ptr(), at, x.data_ptr(), out.data_ptr(), st, ws.data_ptr(), ws.numel()),
                       "axvs_rn_block_fwd")
        return out
