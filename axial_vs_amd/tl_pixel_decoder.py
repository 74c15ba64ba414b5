"""nn.Module mirror of Tube-Link's pixel decoder: `MSDeformAttnPixelDecoder` with the trajectory-attention encoder.

Reference: TL = MaXTron_Tube-Link/mmdet/models/plugins/msdeformattn_pixel_decoder.py:30-325, built from the mmcv config dicts of
`configs/video/{ovis,ytvis21,ytvis22}/*maxtron*` (mmcv 1.6.1 ConvModule / BaseTransformerLayer / DetrTransformerEncoder / FFN).
Same constructor keywords, attribute names and state-dict keys, so `PLUGIN_LAYERS.register_module(name="MSDeformAttnPixelDecoder",
force=True, module=TubeLinkPixelDecoder)` swaps it in and a Tube-Link checkpoint loads with strict=True.

Eval forward: every tensor op runs in libaxvs.so -- input projections (axvs_conv1x1_gn_fwd, straight into the concatenated token
buffer), 2-D sine + level embeddings (axvs_pos2d), 3-D sine + level embeddings (generated inside the trajectory kernels), each encoder
layer's `MultiScaleDeformableAxialTrajectoryAttention` (the existing plugin, reused as is) and FFN tail (axvs_ffn_packed_fwd), then
the FPN tail (axvs_fpn_level_fwd: lateral 1x1 conv + GN + bilinear merge, 3x3 conv + GN + ReLU, mask_feature).  PyTorch only
allocates and transposes the returned maps to NCHW.
train() mode, or inputs that need a gradient: the reference's composition under torch autograd (torch conv / GroupNorm / interpolate /
LayerNorm / Linear around the plugin's own training path) -- not yet the library's HIP training tier.
"""
from __future__ import annotations

import math
from typing import List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from . import _lib
from ._params import conv_gn_params, ffn_params, fpn_level_params
from .modules import PositionEmbeddingSine3D, _cached_pack, _dev_f32, _operand_dtype, _pack_weights, _param_key, _stream, _workspace, _guarded
from .tube_link import MultiScaleDeformableAxialTrajectoryAttention

_ATTN = "MultiScaleDeformableAxialTrajectoryAttention"


def _get(cfg, key, default=None):
    """mmcv config access for plain dicts and attribute-style dicts (mmcv.ConfigDict, TL:99 reads encoder.transformerlayers.attn_cfgs...)."""
    if cfg is None:
        return default
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def _unsupported(field: str, value) -> None:
    raise NotImplementedError(f"axial_vs_amd.TubeLinkPixelDecoder: {field} = {value!r} is not supported (the shipped Tube-Link MaXTron "
                              "configs use MultiScaleDeformableAxialTrajectoryAttention, ('self_attn', 'norm', 'ffn', 'norm'), a 2-fc ReLU FFN, "
                              "GN(32) and ReLU)")


class _ConvModule(nn.Module):
    """mmcv ConvModule(conv -> gn -> act) parameter holder: `conv` (Conv2d) and `gn` (GroupNorm), the reference's names."""

    def __init__(self, cin: int, cout: int, k: int, bias: bool, groups: int, act: bool):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, stride=1, padding=k // 2, bias=bias)
        self.gn = nn.GroupNorm(groups, cout)
        self.with_activation = act

    def forward(self, x: Tensor) -> Tensor:
        x = self.gn(self.conv(x))
        return F.relu(x) if self.with_activation else x


class _FFN(nn.Module):
    """mmcv FFN(num_fcs=2, ReLU, add_identity): layers = Sequential(Sequential(Linear, ReLU, Dropout), Linear, Dropout)."""

    def __init__(self, C: int, F_: int, drop: float):
        super().__init__()
        self.layers = nn.Sequential(nn.Sequential(nn.Linear(C, F_), nn.ReLU(inplace=True), nn.Dropout(drop)), nn.Linear(F_, C), nn.Dropout(drop))

    def forward(self, x: Tensor) -> Tensor:
        return x + self.layers(x)


class _EncoderLayer(nn.Module):
    """mmcv BaseTransformerLayer with operation_order ('self_attn', 'norm', 'ffn', 'norm'): attentions / ffns / norms."""

    def __init__(self, attn: nn.Module, C: int, F_: int, drop: float):
        super().__init__()
        self.attentions = nn.ModuleList([attn])
        self.ffns = nn.ModuleList([_FFN(C, F_, drop)])
        self.norms = nn.ModuleList([nn.LayerNorm(C), nn.LayerNorm(C)])


class _Encoder(nn.Module):
    """DetrTransformerEncoder (post-norm: no extra norm): `layers`."""

    def __init__(self, layers: List[nn.Module]):
        super().__init__()
        self.layers = nn.ModuleList(layers)
        self.num_layers = len(layers)


class TubeLinkPixelDecoder(nn.Module):
    def __init__(self, in_channels=(256, 512, 1024, 2048), strides=(4, 8, 16, 32), feat_channels=256, out_channels=256, num_outs=3,
                 norm_cfg=None, act_cfg=None, encoder=None, positional_encoding=None, init_cfg=None, mfma_dtype: Optional[str] = None):
        super().__init__()
        norm_cfg = dict(type="GN", num_groups=32) if norm_cfg is None else norm_cfg
        act_cfg = dict(type="ReLU") if act_cfg is None else act_cfg
        if encoder is None:
            raise NotImplementedError("axial_vs_amd.TubeLinkPixelDecoder: pass the config's `encoder` dict")
        positional_encoding = dict(type="SinePositionalEncoding", num_feats=128, normalize=True) if positional_encoding is None else positional_encoding
        if _get(norm_cfg, "type") != "GN":
            _unsupported("norm_cfg.type", _get(norm_cfg, "type"))
        if _get(act_cfg, "type") != "ReLU":
            _unsupported("act_cfg.type", _get(act_cfg, "type"))
        if feat_channels != 256:
            _unsupported("feat_channels", feat_channels)
        if out_channels % 32:
            _unsupported("out_channels", out_channels)
        groups = _get(norm_cfg, "num_groups", 32)
        if groups != 32:
            _unsupported("norm_cfg.num_groups", groups)
        tl = _get(encoder, "transformerlayers")
        attn_cfg = _get(tl, "attn_cfgs")
        if isinstance(attn_cfg, (list, tuple)):
            if len(attn_cfg) != 1:
                _unsupported("encoder.transformerlayers.attn_cfgs", attn_cfg)
            attn_cfg = attn_cfg[0]
        if _get(attn_cfg, "type") != _ATTN:
            _unsupported("encoder.transformerlayers.attn_cfgs.type", _get(attn_cfg, "type"))
        order = tuple(_get(tl, "operation_order", ()))
        if order != ("self_attn", "norm", "ffn", "norm"):
            _unsupported("encoder.transformerlayers.operation_order", order)
        ffn_cfgs = _get(tl, "ffn_cfgs")
        if ffn_cfgs is not None:
            if _get(ffn_cfgs, "num_fcs", 2) != 2:
                _unsupported("encoder.transformerlayers.ffn_cfgs.num_fcs", _get(ffn_cfgs, "num_fcs"))
            act = _get(_get(ffn_cfgs, "act_cfg", {}), "type", "ReLU")
            if act != "ReLU":
                _unsupported("encoder.transformerlayers.ffn_cfgs.act_cfg.type", act)
        if _get(positional_encoding, "type", "SinePositionalEncoding") != "SinePositionalEncoding":
            _unsupported("positional_encoding.type", _get(positional_encoding, "type"))
        num_feats = _get(positional_encoding, "num_feats", 128)
        if 2 * num_feats != feat_channels or not _get(positional_encoding, "normalize", False) or _get(positional_encoding, "offset", 0.0) != 0.0:
            _unsupported("positional_encoding", positional_encoding)

        self.strides = list(strides)
        self.num_input_levels = len(in_channels)
        self.num_encoder_levels = _get(attn_cfg, "num_levels")                                        # TL:98-101
        assert self.num_encoder_levels >= 1, "num_levels in attn_cfgs must be at least one"
        if self.num_encoder_levels >= self.num_input_levels:
            _unsupported("num_levels (every input level in the encoder: no FPN level for mask_feature)", self.num_encoder_levels)
        self.use_temporal_attn = True
        self.num_temporal_levels = _get(attn_cfg, "num_temporal_levels", 2)
        self.level_3d_encodeing = nn.Embedding(self.num_temporal_levels, feat_channels)                   # (the reference's spelling)
        self.feat_channels, self.out_channels, self.groups = feat_channels, out_channels, groups
        self.input_convs = nn.ModuleList([_ConvModule(in_channels[i], feat_channels, 1, True, groups, False)     # TL:108-120
                                          for i in range(self.num_input_levels - 1, self.num_input_levels - self.num_encoder_levels - 1, -1)])
        num_layers = _get(encoder, "num_layers", 6)
        d_ffn = _get(tl, "feedforward_channels", None)
        if d_ffn is None:
            d_ffn = _get(ffn_cfgs, "feedforward_channels", 1024)
        ffn_drop = _get(tl, "ffn_dropout", None)
        if ffn_drop is None:
            ffn_drop = _get(ffn_cfgs, "ffn_drop", 0.0)
        akw = {k: _get(attn_cfg, k) for k in ("embed_dims", "num_heads", "num_levels", "num_temporal_levels", "num_temporal_layers",
                                              "num_temporal_dim", "num_points", "im2col_step", "dropout", "batch_first", "skip_connect",
                                              "attn_drop", "norm_cfg") if _get(attn_cfg, k) is not None}
        if akw.get("embed_dims", 256) != feat_channels:
            _unsupported("attn_cfgs.embed_dims", akw.get("embed_dims"))
        self.encoder = _Encoder([_EncoderLayer(MultiScaleDeformableAxialTrajectoryAttention(mfma_dtype=mfma_dtype, **akw), feat_channels, d_ffn,
                                               ffn_drop) for _ in range(num_layers)])
        self.d_ffn = d_ffn
        self.num_feats = num_feats
        self.temperature = float(_get(positional_encoding, "temperature", 10000))
        self.pos_scale = float(_get(positional_encoding, "scale", 2 * math.pi))
        self.positional_encoding3d = PositionEmbeddingSine3D(num_feats, normalize=True)                  # TL:124
        self.level_encoding = nn.Embedding(self.num_encoder_levels, feat_channels)                        # TL:126-127
        self.use_bias = False                                                                              # norm_cfg is not None (TL:132)
        self.lateral_convs = nn.ModuleList()
        self.output_convs = nn.ModuleList()
        for i in range(self.num_input_levels - self.num_encoder_levels - 1, -1, -1):                       # TL:135-153
            self.lateral_convs.append(_ConvModule(in_channels[i], feat_channels, 1, False, groups, False))
            self.output_convs.append(_ConvModule(feat_channels, feat_channels, 3, False, groups, True))
        self.mask_feature = nn.Conv2d(feat_channels, out_channels, kernel_size=1, stride=1, padding=0)  # TL:155-156
        self.num_outs = num_outs
        self.mfma_dtype = mfma_dtype
        self._pos_cache = None
        self._record_layers = None      # a list: eval forwards append each encoder layer's output rows [BT, S, C] (tests)
        self.init_weights()

    # ------------------------------------------------------------------ init (TL:161-185)
    def init_weights(self) -> None:
        for i in range(self.num_encoder_levels):                   # mmcv xavier_init(gain=1, bias=0, distribution='uniform')
            nn.init.xavier_uniform_(self.input_convs[i].conv.weight, gain=1)
            nn.init.constant_(self.input_convs[i].conv.bias, 0)
        for i in range(self.num_input_levels - self.num_encoder_levels):     # caffe2_xavier_init: kaiming_uniform_(a=1, fan_in, leaky_relu)
            for conv in (self.lateral_convs[i].conv, self.output_convs[i].conv):
                nn.init.kaiming_uniform_(conv.weight, a=1, mode="fan_in", nonlinearity="leaky_relu")
        nn.init.kaiming_uniform_(self.mask_feature.weight, a=1, mode="fan_in", nonlinearity="leaky_relu")
        nn.init.constant_(self.mask_feature.bias, 0)
        nn.init.normal_(self.level_encoding.weight, mean=0, std=1)  # normal_init(level_encoding): the Embedding has no bias
        for p in self.encoder.parameters():
            if p.dim() > 1:
                nn.init.xavier_normal_(p)
        # TL:182-185 re-initialises attentions that are `MultiScaleDeformableAttention` instances; the trajectory plugin is not one,
        # so it keeps the xavier_normal_ sweep above (the reference's behaviour, restated as is)

    # ------------------------------------------------------------------ packs
    _dtype = _operand_dtype

    def _pack_input(self, i: int) -> Tensor:
        m = self.input_convs[i]
        return _cached_pack(self, f"in{i}", self._dtype(), (m,), lambda dt: _pack_weights(
            "axvs_conv1x1_gn", _lib.AxvsConvGnParams, conv_gn_params(m.conv, m.gn), (m.conv.in_channels, m.conv.out_channels), dt))

    def _pack_ffn(self, k: int) -> Tensor:
        layer = self.encoder.layers[k]
        return _cached_pack(self, f"ffn{k}", self._dtype(), (layer.ffns[0], layer.norms), lambda dt: _pack_weights(
            "axvs_ffn", _lib.AxvsFfnParams, ffn_params(layer), (self.feat_channels, self.d_ffn), dt))

    def _pack_fpn(self, i: int) -> Tensor:
        lat, out = self.lateral_convs[i], self.output_convs[i]
        mask = self.mask_feature if i == 0 else None          # the finest level carries the mask head
        return _cached_pack(self, f"fpn{i}", self._dtype(), (lat, out) + ((mask,) if i == 0 else ()), lambda dt: _pack_weights(
            "axvs_fpn_level", _lib.AxvsFpnLevelParams, fpn_level_params(lat, out, mask),
            (lat.conv.in_channels, self.feat_channels, self.out_channels if i == 0 else 0), dt))

    # ------------------------------------------------------------------ forward (TL:187-325)
    def _check_inputs(self, feats) -> None:
        """The reference's conv2d shape errors, raised before any library call (a pack is sized for its module's in_channels)."""
        if len(feats) != self.num_input_levels:
            raise RuntimeError(f"expected {self.num_input_levels} feature maps (in_channels), got {len(feats)}")
        for i in range(self.num_encoder_levels):
            l, want = self.num_input_levels - i - 1, self.input_convs[i].conv.in_channels
            if feats[l].dim() != 4 or feats[l].shape[1] != want:
                raise RuntimeError(f"input_convs[{i}] expects feats[{l}] with {want} channels, got shape {tuple(feats[l].shape)}")
        for i in range(self.num_input_levels - self.num_encoder_levels - 1, -1, -1):      # the order of TL:305
            want = self.lateral_convs[i].conv.in_channels
            if feats[i].dim() != 4 or feats[i].shape[1] != want:
                raise RuntimeError(f"lateral_convs[{i}] expects feats[{i}] with {want} channels, got shape {tuple(feats[i].shape)}")

    @_guarded
    def forward(self, feats: List[Tensor], num_frames: int):
        self._check_inputs(feats)
        if self.training or (torch.is_grad_enabled() and any(f.requires_grad for f in feats)):
            return self._forward_torch(feats, num_frames)
        return self._forward_hip(feats, num_frames)

    def _enc_shapes(self, feats):
        idx = [self.num_input_levels - i - 1 for i in range(self.num_encoder_levels)]     # coarsest first
        return idx, [(int(feats[l].shape[-2]), int(feats[l].shape[-1])) for l in idx]

    @staticmethod
    def _reference_points(shapes, device) -> Tensor:
        """MlvlPointGenerator.single_level_grid_priors (offset 0.5) / (w, h) * stride: ((x + 0.5) / w, (y + 0.5) / h), TL:232-236."""
        pts = []
        for h, w in shapes:
            ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=device), torch.arange(w, dtype=torch.float32, device=device),
                                    indexing="ij")
            pts.append(torch.stack(((xs.reshape(-1) + 0.5) / w, (ys.reshape(-1) + 0.5) / h), -1))
        return torch.cat(pts, 0)

    def _positions(self, BT: int, B: int, T: int, shapes, device):
        """(2-D sine + level_encoding as [BT, S, C] tokens, [3-D sine + level_3d_encodeing per temporal level], reference points,
        spatial shapes, level start index): cached per shape and embedding version, like the within-clip decoder's _pos_cache."""
        key = (BT, T, tuple(shapes), str(device), _param_key(self.level_encoding, "f32"), _param_key(self.level_3d_encodeing, "f32"))
        if self._pos_cache is not None and self._pos_cache[0] == key:
            return self._pos_cache[1]
        Cc = self.feat_channels
        S = sum(h * w for h, w in shapes)
        pos = torch.empty(BT, S, Cc, dtype=torch.float32, device=device)
        lv = _dev_f32(self.level_encoding.weight.detach(), "level_encoding")
        row0 = 0
        for i, (h, w) in enumerate(shapes):
            _lib.check(_lib.lib().axvs_pos2d(pos.data_ptr(), lv[i].data_ptr(), BT, h, w, Cc, S, row0, self.temperature, 1, self.pos_scale,
                                             _stream(device)), "axvs_pos2d")
            row0 += h * w
        lv3 = _dev_f32(self.level_3d_encodeing.weight.detach(), "level_3d_encodeing")
        pos3d = [self.positional_encoding3d.channels_last_with_level(B, T, h, w, lv3[i]) for i, (h, w) in enumerate(shapes[:self.num_temporal_levels])]
        ref = self._reference_points(shapes, device)
        ref = ref[None, :, None].repeat(BT, 1, self.num_encoder_levels, 1).contiguous()
        ss = torch.as_tensor(shapes, dtype=torch.long, device=device)
        lsi = torch.cat((ss.new_zeros((1,)), ss.prod(1).cumsum(0)[:-1]))
        val = (pos, pos3d, ref, ss, lsi)
        self._pos_cache = (key, val)
        return val

    @torch.no_grad()
    def _forward_hip(self, feats, num_frames):
        L = _lib.lib()
        BT = int(feats[0].shape[0])
        T = int(num_frames)
        if T <= 0 or BT % T:
            raise RuntimeError(f"batch {BT} is not a multiple of num_frames {T}")
        B = BT // T
        xs = [_dev_f32(f, "feats") for f in feats]
        dev = xs[0].device
        st = _stream(dev)
        dt = _lib.DTYPES[self._dtype()]
        Cc = self.feat_channels
        idx, shapes = self._enc_shapes(xs)
        S = sum(h * w for h, w in shapes)
        starts = [0]
        for h, w in shapes[:-1]:
            starts.append(starts[-1] + h * w)
        src = torch.empty(BT, S, Cc, dtype=torch.float32, device=dev)
        for i, l in enumerate(idx):                     # input_convs[i] -> token rows of level i, written in place (TL:201-204, 243-244)
            h, w = shapes[i]
            cin = xs[l].shape[1]
            pk = self._pack_input(i)
            ws = _workspace(dev, L.axvs_conv1x1_gn_workspace_bytes(BT, h * w, max(cin, Cc), self.groups), st)
            _lib.check(L.axvs_conv1x1_gn_fwd(xs[l].data_ptr(), 0, 0, 0, src.data_ptr() + starts[i] * Cc * 4, 1, S * Cc, Cc, pk.data_ptr(), BT, h * w,
                                             cin, Cc, self.groups, 1e-5, dt, ws.data_ptr(), ws.numel(), st), "axvs_conv1x1_gn_fwd")
        pos, pos3d, ref, ss, lsi = self._positions(BT, B, T, shapes, dev)
        M = BT * S
        x = src
        for k, layer in enumerate(self.encoder.layers):            # BaseTransformerLayer: self_attn -> norm -> ffn -> norm
            a = layer.attentions[0](x.permute(1, 0, 2) if not layer.attentions[0].batch_first else x, query_pos=pos.permute(1, 0, 2)
                                    if not layer.attentions[0].batch_first else pos, query_pos3d=pos3d, reference_points=ref, spatial_shapes=ss,
                                    level_start_index=lsi)
            a = a.permute(1, 0, 2) if not layer.attentions[0].batch_first else a
            a = a.contiguous()
            out = torch.empty_like(a)
            if self._record_layers is not None:
                self._record_layers.append(out)
            pk = self._pack_ffn(k)
            ws = _workspace(dev, L.axvs_ffn_workspace_bytes(M, Cc, self.d_ffn), st)
            _lib.check(L.axvs_ffn_packed_fwd(a.data_ptr(), out.data_ptr(), pk.data_ptr(), M, Cc, self.d_ffn, dt, ws.data_ptr(), ws.numel(), st),
                       "axvs_ffn_packed_fwd")
            x = out
        # encoder levels as NCHW maps, low to high resolution (TL:293-303)
        outs = [x[:, starts[i]:starts[i] + h * w].transpose(1, 2).reshape(BT, Cc, h, w) for i, (h, w) in enumerate(shapes)]
        up, up_bs, (Hu, Wu) = x.data_ptr() + starts[-1] * Cc * 4, S * Cc, shapes[-1]
        keep = []
        mask_feature = None
        n_fpn = self.num_input_levels - self.num_encoder_levels
        for j, i in enumerate(range(n_fpn - 1, -1, -1)):           # TL:305-320, the reference's indexing: lateral_convs[i] / output_convs[i]
            xi = xs[i]
            H, W = int(xi.shape[-2]), int(xi.shape[-1])
            cin = int(xi.shape[1])
            last = i == 0
            want_y = not last or len(outs) < self.num_outs
            y = torch.empty(BT, H * W, Cc, dtype=torch.float32, device=dev) if want_y else None
            mf = torch.empty(BT, self.out_channels, H, W, dtype=torch.float32, device=dev) if last else None
            pk = self._pack_fpn(i)
            ws = _workspace(dev, L.axvs_fpn_level_workspace_bytes(BT, H, W, cin, Cc, self.groups), st)
            _lib.check(L.axvs_fpn_level_fwd(xi.data_ptr(), up, up_bs, Cc, Hu, Wu, y.data_ptr() if y is not None else None,
                                            mf.data_ptr() if mf is not None else None, pk.data_ptr(), BT, H, W, cin, Cc,
                                            self.out_channels if i == 0 else 0, self.groups, 1e-5, dt, ws.data_ptr(), ws.numel(), st),
                       "axvs_fpn_level_fwd")
            if y is not None:
                keep.append(y)
                outs.append(y.transpose(1, 2).reshape(BT, Cc, H, W))
                up, up_bs, Hu, Wu = y.data_ptr(), H * W * Cc, H, W
            else:
                outs.append(None)
            mask_feature = mf
        multi_scale_features = [o.contiguous() for o in outs[:self.num_outs]]
        return mask_feature, multi_scale_features

    def _forward_torch(self, feats, num_frames):
        """The reference's forward (TL:187-325) under torch autograd: torch conv / GroupNorm / interpolate / LayerNorm / Linear around the
        plugin's training path.  Not yet the library's HIP training tier."""
        BT = int(feats[0].shape[0])
        T = int(num_frames)
        B = BT // T
        idx, shapes = self._enc_shapes(feats)
        dev = feats[0].device
        srcs, poss = [], []
        for i, l in enumerate(idx):
            h, w = shapes[i]
            f = self.input_convs[i](feats[l])
            srcs.append(f.flatten(2).transpose(1, 2))
            poss.append(_sine2d(h, w, self.num_feats, self.temperature, self.pos_scale, dev).to(f.dtype)[None] + self.level_encoding.weight[i])
        src = torch.cat(srcs, 1)
        pos = torch.cat(poss, 1).expand(BT, -1, -1)
        with torch.no_grad():
            pos3d_raw = [self.positional_encoding3d.channels_last(B, T, h, w, dev) for h, w in shapes[:self.num_temporal_levels]]
        pos3d = [p.to(src.dtype) + self.level_3d_encodeing.weight[i] for i, p in enumerate(pos3d_raw)]
        ref = self._reference_points(shapes, dev).to(src.dtype)[None, :, None].repeat(BT, 1, self.num_encoder_levels, 1)
        ss = torch.as_tensor(shapes, dtype=torch.long, device=dev)
        lsi = torch.cat((ss.new_zeros((1,)), ss.prod(1).cumsum(0)[:-1]))
        x = src
        for layer in self.encoder.layers:
            attn = layer.attentions[0]
            q, p = (x, pos) if attn.batch_first else (x.transpose(0, 1), pos.transpose(0, 1))
            a = attn(q, query_pos=p, query_pos3d=pos3d, reference_points=ref, spatial_shapes=ss, level_start_index=lsi)
            a = a if attn.batch_first else a.transpose(0, 1)
            x = layer.norms[1](layer.ffns[0](layer.norms[0](a)))
        outs = [o.transpose(1, 2).reshape(BT, self.feat_channels, h, w) for o, (h, w) in zip(torch.split(x, [h * w for h, w in shapes], 1), shapes)]
        for i in range(self.num_input_levels - self.num_encoder_levels - 1, -1, -1):
            cur = self.lateral_convs[i](feats[i])
            y = cur + F.interpolate(outs[-1], size=cur.shape[-2:], mode="bilinear", align_corners=False)
            outs.append(self.output_convs[i](y))
        return self.mask_feature(outs[-1]), outs[:self.num_outs]


def _sine2d(h: int, w: int, num_feats: int, temperature: float, scale: float, device) -> Tensor:
    """mmdet SinePositionalEncoding(num_feats, normalize=True, offset=0, eps=1e-6) of an all-valid mask, as [h*w, 2*num_feats] tokens."""
    y = torch.arange(1, h + 1, dtype=torch.float32, device=device)[:, None].expand(h, w)
    x = torch.arange(1, w + 1, dtype=torch.float32, device=device)[None, :].expand(h, w)
    y = y / (h + 1e-6) * scale
    x = x / (w + 1e-6) * scale
    dim_t = torch.arange(num_feats, dtype=torch.float32, device=device)
    dim_t = temperature ** (2 * (dim_t // 2) / num_feats)
    px, py = x[..., None] / dim_t, y[..., None] / dim_t
    px = torch.stack((px[..., 0::2].sin(), px[..., 1::2].cos()), dim=-1).flatten(2)
    py = torch.stack((py[..., 0::2].sin(), py[..., 1::2].cos()), dim=-1).flatten(2)
    return torch.cat((py, px), -1).reshape(h * w, 2 * num_feats)
