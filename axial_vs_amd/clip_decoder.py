"""Tube-Link's per-clip masked-attention query decoder on the device.

Reference (MaXTron_Tube-Link): `Mask2FormerVideoCCHeadTube.forward` (models/video/tube_link_vis/mask2former_video_cc_head.py:840-903) with
`forward_head_video` (:738-759): per clip, nine `DetrTransformerDecoderLayer`s (masked cross-attention to one of three memory levels,
self-attention, FFN), each behind a mask head that thresholds the current mask prediction into the attention mask.  The head freezes
this decoder and keeps it in eval() in training and inference alike (:411-422, :819-820), so the path is forward only.

The reference computes the stride-4 mask prediction in front of every layer and bilinearly shrinks it to the level's size just to
threshold it.  Both steps are linear, so here the mask features are resized once per level and the mask logits are computed at level
resolution: `mask_embed . resize(mask_feature)`; the attention mask is one bit per (clip, query, key), read by all eight heads.  The
full-resolution einsum runs once, and only with `return_predictions=True`.  All clips of a step can be stacked into one call.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from . import _lib
from ._params import m2f_head_params, m2f_layer_params
from .matching import match_clips
from .modules import _cached_pack, _dev_f32, _guarded, _pack_folded, _stream, _workspace_for

_ORDER = ("cross_attn", "norm", "self_attn", "norm", "ffn", "norm")


class _Attention(nn.Module):
    """mmcv's MultiheadAttention wrapper: the parameters live in `.attn` (nn.MultiheadAttention)"""

    def __init__(self, c: int, heads: int):
        super().__init__()
        self.attn = nn.MultiheadAttention(c, heads, dropout=0.0)


class _FFN(nn.Module):
    """mmcv's FFN: layers = Sequential(Sequential(Linear, ReLU, Dropout), Linear, Dropout)"""

    def __init__(self, c: int, f: int):
        super().__init__()
        self.layers = nn.Sequential(nn.Sequential(nn.Linear(c, f), nn.ReLU(inplace=True), nn.Dropout(0.0)), nn.Linear(f, c), nn.Dropout(0.0))


class _DecoderLayer(nn.Module):
    def __init__(self, c: int, heads: int, f: int):
        super().__init__()
        self.attentions = nn.ModuleList([_Attention(c, heads), _Attention(c, heads)])
        self.ffns = nn.ModuleList([_FFN(c, f)])
        self.norms = nn.ModuleList([nn.LayerNorm(c) for _ in range(3)])


def _nonzero(cfg: dict, *names) -> bool:
    return any(float(cfg.get(n) or 0.0) != 0.0 for n in names)


def _check_decoder_cfg(cfg: dict, feat_channels: int) -> Tuple[int, int, int]:
    """(num_layers, heads, FFN width) of a `DetrTransformerDecoder` config, or NotImplementedError for what has no device path"""
    lay = cfg.get("transformerlayers") or {}
    if isinstance(lay, (list, tuple)):
        raise NotImplementedError("axial_vs_amd: per-layer transformerlayers configs have no HIP path")
    order = tuple(lay.get("operation_order") or ())
    if order != _ORDER:
        raise NotImplementedError(f"axial_vs_amd: operation_order {order} has no HIP path (pre-norm included); the decoder kernels run {_ORDER}")
    attn = lay.get("attn_cfgs") or {}
    if isinstance(attn, (list, tuple)):
        raise NotImplementedError("axial_vs_amd: per-attention attn_cfgs have no HIP path")
    ffn = lay.get("ffn_cfgs") or {}
    if _nonzero(attn, "attn_drop", "proj_drop", "dropout") or _nonzero(ffn, "ffn_drop", "dropout") or \
            (attn.get("dropout_layer") or {}).get("drop_prob") or (ffn.get("dropout_layer") or {}).get("drop_prob"):
        raise NotImplementedError("axial_vs_amd: the decoder kernels have no dropout (the reference's configuration: every rate 0)")
    if attn.get("batch_first"):
        raise NotImplementedError("axial_vs_amd: batch_first attention has no HIP path")
    act = (ffn.get("act_cfg") or {"type": "ReLU"}).get("type")
    if act != "ReLU" or int(ffn.get("num_fcs", 2)) != 2 or not ffn.get("add_identity", True):
        raise NotImplementedError("axial_vs_amd: the decoder FFN is Linear-ReLU-Linear with identity")
    heads = int(attn.get("num_heads", 8))
    f = int(ffn.get("feedforward_channels", lay.get("feedforward_channels", 2048)))
    if int(attn.get("embed_dims", feat_channels)) != feat_channels or int(ffn.get("embed_dims", feat_channels)) != feat_channels:
        raise NotImplementedError("axial_vs_amd: embed_dims of the decoder layers must equal feat_channels")
    return int(cfg.get("num_layers", 9)), heads, f


class TubeLinkClipDecoder(nn.Module):
    """The per-clip query decoder of `Mask2FormerVideoCCHeadTube` under the head's own parameter names -- a checkpoint of the head loads
    with strict=False and fills every parameter here.  Keyword names follow the head's constructor.

    forward(mask_features [N,T,C,h,w], multi_scale_memorys: three [N,T,C,h_l,w_l], low to high resolution, return_predictions=False)
        -> query_feat [Q,N,C] after the last layer (what :903 collects per clip); with return_predictions also the last layer's
           cls_pred [N,Q,K+1] and mask_pred [N,T,Q,h,w].
    N counts (video, clip) pairs: clips are independent, so all clips of a step may be stacked.  GPU tensors only; forward only (the head
    keeps this decoder frozen and in eval() mode)."""

    def __init__(self, num_queries: int, num_classes: int, feat_channels: int = 256, out_channels: int = 256,
                 transformer_decoder: Optional[dict] = None, positional_encoding: Optional[dict] = None, num_transformer_feat_level: int = 3,
                 enforce_decoder_input_project: bool = False):
        super().__init__()
        if enforce_decoder_input_project:
            raise NotImplementedError("axial_vs_amd: decoder_input_projs must be identities (enforce_decoder_input_project=False)")
        if feat_channels != 256 or out_channels != 256:
            raise NotImplementedError("axial_vs_amd: the decoder kernels are built for feat_channels = out_channels = 256")
        if num_transformer_feat_level != 3:
            raise NotImplementedError("axial_vs_amd: the decoder kernels are built for 3 memory levels")
        if transformer_decoder is None:
            transformer_decoder = dict(num_layers=9, transformerlayers=dict(
                attn_cfgs=dict(embed_dims=256, num_heads=8), ffn_cfgs=dict(embed_dims=256, feedforward_channels=2048), operation_order=_ORDER))
        nl, heads, f = _check_decoder_cfg(transformer_decoder, feat_channels)
        if heads != 8 or f != 2048 or not 1 <= nl <= 16:
            raise NotImplementedError(f"axial_vs_amd: the decoder kernels are built for 8 heads, FFN 2048 and 1..16 layers (got {heads}, {f}, {nl})")
        pe = dict(positional_encoding or dict(num_feats=128, normalize=True))
        if int(pe.get("num_feats", 128)) * 2 != feat_channels or float(pe.get("offset", 0.0)) != 0.0 or float(pe.get("eps", 1e-6)) != 1e-6:
            raise NotImplementedError("axial_vs_amd: SinePositionalEncoding3D needs num_feats = feat_channels / 2, offset 0, eps 1e-6")
        if not 1 <= num_queries <= 256:
            raise NotImplementedError("axial_vs_amd: the decoder kernels take 1..256 queries")
        self.pos_temperature = float(pe.get("temperature", 10000))
        self.pos_normalize = bool(pe.get("normalize", False))
        self.pos_scale = float(pe.get("scale", 2 * 3.141592653589793))
        self.num_queries, self.num_classes, self.num_layers = num_queries, num_classes, nl
        self.num_heads, self.feedforward_channels, self.num_transformer_feat_level = heads, f, 3
        self.transformer_decoder = nn.Module()
        self.transformer_decoder.layers = nn.ModuleList([_DecoderLayer(feat_channels, heads, f) for _ in range(nl)])
        self.transformer_decoder.post_norm = nn.LayerNorm(feat_channels)
        self.query_embed = nn.Embedding(num_queries, feat_channels)
        self.query_feat = nn.Embedding(num_queries, feat_channels)
        self.level_embed = nn.Embedding(3, feat_channels)
        self.cls_embed = nn.Linear(feat_channels, num_classes + 1)
        self.mask_embed = nn.Sequential(nn.Linear(feat_channels, feat_channels), nn.ReLU(inplace=True),
                                        nn.Linear(feat_channels, feat_channels), nn.ReLU(inplace=True),
                                        nn.Linear(feat_channels, out_channels))

    def train(self, mode: bool = True):
        return super().train(False)      # the head keeps this decoder in eval() whatever its own mode (TLCC:819-820)

    # ---- the library's view ----
    def _cfg(self, N: int, T: int, h: int, w: int, sizes: Sequence[Tuple[int, int]], return_predictions: bool = False) -> _lib.AxvsM2fCfg:
        return _lib.AxvsM2fCfg(N=N, Q=self.num_queries, T=T, C=256, heads=self.num_heads, ffn=self.feedforward_channels, num_layers=self.num_layers,
                               num_levels=3, K1=self.num_classes + 1, h=h, w=w, lh=(C.c_int * 3)(*[int(s[0]) for s in sizes]),
                               lw=(C.c_int * 3)(*[int(s[1]) for s in sizes]), return_predictions=int(return_predictions),
                               pos_normalize=int(self.pos_normalize), pos_temperature=self.pos_temperature, pos_scale=self.pos_scale)

    def _pack(self) -> Tensor:
        def build(dt):      # (nothing to fold: the parameters themselves, refused one by one when they are not on the GPU)
            layers = [[_dev_f32(t.detach(), "parameter") for t in m2f_layer_params(lay)] for lay in self.transformer_decoder.layers]
            head = [_dev_f32(t.detach(), "parameter") for t in m2f_head_params(self)]
            return _pack_folded("axvs_m2f_decoder", self._cfg(1, 1, 1, 1, [(1, 1)] * 3), [(_lib.AxvsM2fLayerParams, layers), (_lib.AxvsM2fHeadParams, [head])])
        return _cached_pack(self, "m2f", "f32", (self,), build)

    def _inputs(self, mask_features: Tensor, memorys: Sequence[Tensor]):
        mf = _dev_f32(mask_features, "mask_features")
        if mf.dim() != 5 or mf.shape[2] != 256 or len(memorys) != 3:
            raise RuntimeError(f"mask_features {tuple(mf.shape)} must be [N,T,256,h,w] with three memory levels (got {len(memorys)})")
        mems = [_dev_f32(m, "multi_scale_memorys") for m in memorys]
        for m in mems:
            if m.dim() != 5 or m.shape[:3] != mf.shape[:3]:
                raise RuntimeError(f"memory {tuple(m.shape)} must be [N,T,256,h_l,w_l] with the mask features' N = {mf.shape[0]}, T = {mf.shape[1]}")
        return mf, mems

    @_guarded
    @torch.no_grad()
    def forward(self, mask_features: Tensor, multi_scale_memorys: Sequence[Tensor], return_predictions: bool = False, return_masks: bool = False):
        """`return_masks=True` (a debugging aid, what the tests read) appends every layer's attention mask as the layer consumed it:
        a list of (bits int32 [N,Q,ceil(S_l/32)], flags int32 [N,Q]); bit k & 31 of word k / 32 set = key k masked, flag 0 = every key
        masked (the query then attends to all keys)."""
        mf, mems = self._inputs(mask_features, multi_scale_memorys)
        N, T, _, h, w = mf.shape
        sizes = [tuple(m.shape[-2:]) for m in mems]
        cfg = self._cfg(N, T, h, w, sizes, return_predictions)
        L, dev, Q, nl = _lib.lib(), mf.device, self.num_queries, self.num_layers
        packed = self._pack()
        st = _stream(dev)
        ws = _workspace_for("axvs_m2f_decoder_workspace_bytes", dev, st, C.byref(cfg))
        out = torch.empty(N, Q, 256, dtype=torch.float32, device=dev)
        cls = torch.empty(N, Q, self.num_classes + 1, dtype=torch.float32, device=dev) if return_predictions else None
        masks = torch.empty(N, T, Q, h, w, dtype=torch.float32, device=dev) if return_predictions else None
        words = [(T * sizes[i % 3][0] * sizes[i % 3][1] + 31) // 32 for i in range(nl)]
        dbits = torch.empty(N * Q * sum(words), dtype=torch.int32, device=dev) if return_masks else None
        dflags = torch.empty(nl, N, Q, dtype=torch.int32, device=dev) if return_masks else None
        ptr = lambda t: None if t is None else t.data_ptr()
        mp = (C.c_void_p * 3)(*[m.data_ptr() for m in mems])
        _lib.check(L.axvs_m2f_decoder_fwd(C.byref(cfg), packed.data_ptr(), mf.data_ptr(), mp, out.data_ptr(), ptr(cls), ptr(masks), ptr(dbits), ptr(dflags),
                                          ws.data_ptr(), ws.numel(), st), "axvs_m2f_decoder_fwd")
        res = [out.transpose(0, 1)]      # [Q,N,C], the reference's layout
        if return_predictions:
            res += [cls, masks]
        if return_masks:
            lm, o = [], 0
            for i in range(nl):
                lm.append((dbits[o:o + N * Q * words[i]].view(N, Q, words[i]), dflags[i]))
                o += N * Q * words[i]
            res.append(lm)
        return res[0] if len(res) == 1 else tuple(res)

    @_guarded
    @torch.no_grad()
    def attention_mask(self, x: Tensor, mask_features: Tensor, level_size: Tuple[int, int], level: int = 0):
        """One mask head (`forward_head_video` reduced to its attention mask): x [N,Q,C] queries before post_norm ->
        (bits int32 [N,Q,ceil(S/32)], flags int32 [N,Q]) at `level_size` = (h_l, w_l)."""
        x = _dev_f32(x, "x")
        mf = _dev_f32(mask_features, "mask_features")
        N, T, _, h, w = mf.shape
        sizes = [(1, 1)] * 3
        sizes[level] = tuple(level_size)
        cfg = self._cfg(N, T, h, w, sizes)
        L, dev, Q = _lib.lib(), mf.device, self.num_queries
        if x.shape != (N, Q, 256):
            raise RuntimeError(f"x {tuple(x.shape)} must be [N={N},Q={Q},256]")
        packed = self._pack()
        st = _stream(dev)
        ws = _workspace_for("axvs_m2f_attn_mask_workspace_bytes", dev, st, C.byref(cfg), level)
        W = (T * level_size[0] * level_size[1] + 31) // 32
        bits = torch.empty(N, Q, W, dtype=torch.int32, device=dev)
        flags = torch.empty(N, Q, dtype=torch.int32, device=dev)
        _lib.check(L.axvs_m2f_attn_mask_fwd(C.byref(cfg), packed.data_ptr(), x.data_ptr(), mf.data_ptr(), level, bits.data_ptr(), flags.data_ptr(),
                                            ws.data_ptr(), ws.numel(), st), "axvs_m2f_attn_mask_fwd")
        return bits, flags

    @_guarded
    @torch.no_grad()
    def layer(self, x: Tensor, memory: Tensor, bits: Tensor, flags: Tensor, index: int) -> Tensor:
        """Layer `index` given its attention mask: x [N,Q,C], memory [N,T,C,h_l,w_l] of level index % 3, bits / flags as
        `attention_mask` returns them -> [N,Q,C]."""
        x = _dev_f32(x, "x")
        mem = _dev_f32(memory, "memory")
        N, T, _, hl, wl = mem.shape
        sizes = [(1, 1)] * 3
        sizes[index % 3] = (hl, wl)
        cfg = self._cfg(N, T, 1, 1, sizes)
        L, dev, Q = _lib.lib(), mem.device, self.num_queries
        W = (T * hl * wl + 31) // 32
        if x.shape != (N, Q, 256) or bits.shape != (N, Q, W) or flags.shape != (N, Q) or bits.dtype != torch.int32 or flags.dtype != torch.int32:
            raise RuntimeError(f"x {tuple(x.shape)}, bits {tuple(bits.shape)}, flags {tuple(flags.shape)} must be [N,Q,256], int32 [N,Q,{W}], int32 [N,Q]")
        bits, flags = bits.contiguous(), flags.contiguous()
        packed = self._pack()
        st = _stream(dev)
        ws = _workspace_for("axvs_m2f_layer_workspace_bytes", dev, st, C.byref(cfg), index)
        out = torch.empty_like(x)
        _lib.check(L.axvs_m2f_layer_fwd(C.byref(cfg), packed.data_ptr(), index, x.data_ptr(), mem.data_ptr(), bits.data_ptr(), flags.data_ptr(),
                                        out.data_ptr(), ws.data_ptr(), ws.numel(), st), "axvs_m2f_layer_fwd")
        return out


def unpack_mask_bits(bits: Tensor, S: int) -> Tensor:
    """int32 words [..., ceil(S/32)] -> bool [..., S]: True = key masked"""
    sh = torch.arange(32, device=bits.device, dtype=torch.int64)
    return ((((bits.to(torch.int64) & 0xFFFFFFFF).unsqueeze(-1) >> sh) & 1) != 0).flatten(-2)[..., :S]


def pack_mask_bits(mask: Tensor) -> Tensor:
    """bool [..., S] (True = key masked) -> int32 words [..., ceil(S/32)], bits past S zero"""
    S = mask.shape[-1]
    W = (S + 31) // 32
    m = torch.zeros(*mask.shape[:-1], W * 32, dtype=torch.int64, device=mask.device)
    m[..., :S] = mask.to(torch.int64)
    words = (m.view(*mask.shape[:-1], W, 32) << torch.arange(32, device=mask.device, dtype=torch.int64)).sum(-1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def tube_link_clip_queries(decoder: TubeLinkClipDecoder, per_clip_outputs: Sequence[Tuple[Tensor, Sequence[Tensor]]]) -> Tensor:
    """TLCC:835-917 for a whole step: `per_clip_outputs[c]` = the pixel decoder's (mask_features [B,T,C,h,w], three memories
    [B,T,C,h_l,w_l]) of clip c.  All clips are stacked and decoded in one call, then clip i is aligned to the already aligned clip
    i - 1 (`match_clips`: the reference's `match_from_embds` chain).  Returns clip_query [B,Tc,Q,C] for `TubeLinkCrossClipHead`."""
    Tc = len(per_clip_outputs)
    B = per_clip_outputs[0][0].shape[0]
    mf = torch.cat([o[0] for o in per_clip_outputs], dim=0)                                   # row c*B + b
    mems = [torch.cat([o[1][l] for o in per_clip_outputs], dim=0) for l in range(3)]
    q = decoder(mf, mems)                                                                     # [Q, Tc*B, C]
    Q, _, Cc = q.shape
    emb = q.reshape(Q, Tc, B, Cc).permute(2, 1, 0, 3).contiguous()                            # [B,Tc,Q,C]
    return match_clips(emb, emb).permute(0, 2, 1, 3).contiguous()                             # match_clips: [B,Q,Tc,C]
