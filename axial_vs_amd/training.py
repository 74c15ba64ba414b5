"""Training path of TemporalAxialTrajectoryAttentionLayer and of the full T*H*W TemporalTrajectoryAttentionLayer:
autograd over libaxvs.so's training tier (``axvs_traj_layer_train_fwd`` / ``_bwd`` for the full layer: the same pass and tail code, one
pass over all T*H*W tokens of a clip; frames longer than LDS holds run on chunked-key attention kernels), and of the deformable
encoder layer MSDeformAttnTransformerEncoderLayer (``axvs_msda_layer_train_fwd`` / ``_bwd``, ``msda_layer_train``: the same tail and
dropout hash, the deformable attention's sampling head and the library's fp32 core op).

Reference: the layer in ``train()`` mode under autograd, WC/temporal_attention.py:187-220 (and TrajectoryAttention :35-76), as the
shipped configs train it (``ATTN_DROP: 0.1``, AMP -- VK/configs/VIPSeg/.../maxtron_wc_convnext_large.yaml).  The forward and the
backward pass both run in the library (``axvs_axial_layer_train_fwd`` / ``_bwd``: fp32 activations, hand-written attention /
softmax / dropout / LayerNorm kernels, split-precision bf16 MFMA GEMMs for the Linear layers); this file is the ``torch.autograd.Function`` that
binds them, nothing is computed here.

* ``layer.recompute = False`` (default): the activations stay in HBM between forward and backward (~44 C floats per token and layer),
  like the reference under autograd.  ``layer.recompute = True``: the forward pass keeps only (src, pos, seed); backward rebuilds the
  activations first (one more forward, no memory held).
* dropout masks are a counter-based hash of (seed, site, element offset) -- see include/axvs.h -- so they are regenerated, never
  stored; ``seed`` comes from torch's CPU generator (``torch.manual_seed`` makes runs repeatable) or ``layer.dropout_seed``.
* AMP: under ``torch.autocast`` the inputs are cast to fp32 at the boundary and the layer returns fp32 (LayerNorm output is fp32
  under autocast in the reference as well); gradients come back in each input's own dtype, so ``GradScaler`` works unchanged.  The
  Linear layers then multiply ONE 16-bit piece per operand in the autocast dtype (bf16 / fp16, fp32 accumulation) -- what autocast
  gives the reference's ``nn.Linear`` -- in the forward, input-gradient and weight-gradient GEMMs (library option ``train_amp``);
  ``layer.amp_compute = False`` keeps the split-precision (fp32-accurate) products.  Attention, softmax, LayerNorm and bias
  gradients stay fp32.
"""
from __future__ import annotations

import ctypes as C
from typing import List

import torch
from torch import Tensor

from . import _lib
from ._autograd import apply, cast, draw_seed, f32c, grad_buffer, nbytes, place, require_gpu
from ._params import axial_layer_params, msda_layer_params, traj_layer_params

# the parameter lists handed to autograd, in their struct's field order (their names here are part of the tested surface)
layer_parameters = axial_layer_params
traj_layer_parameters = traj_layer_params
msda_layer_parameters = msda_layer_params


# the two layers' entry points: (library symbol prefix, parameter struct); `dims` is the size argument list of each
_AXIAL = ("axvs_axial_layer_train", _lib.AxvsAxialLayerParams)
_FULL = ("axvs_traj_layer_train", _lib.AxvsTrajLayerParams)


class _LayerTrain(torch.autograd.Function):
    """forward / backward of one layer through the library's training tier (`kind`: _AXIAL or _FULL)."""

    @staticmethod
    def forward(ctx, src, pos, kind, dims, p_dropout, p_attn_drop, seed, recompute, *params):
        from .modules import _stream
        name, struct = kind
        require_gpu(src)
        s, p = f32c(src), f32c(pos)
        ws = [f32c(w) for w in params]
        dev = s.device
        nsaved = nbytes(name + "_saved_bytes", *dims)
        with torch.cuda.device(dev):
            out = torch.empty_like(s)
            nscr = nbytes(name + "_scratch_bytes", *dims, 0)
            saved, saved_ptr, scratch = place(dev, nsaved, nscr, recompute)
            st = _lib.fill(struct, [w.data_ptr() for w in ws])
            _lib.check(getattr(_lib.lib(), name + "_fwd")(s.data_ptr(), p.data_ptr(), out.data_ptr(), C.byref(st), *dims, float(p_dropout),
                                                          float(p_attn_drop), int(seed), saved_ptr, nsaved, scratch.data_ptr(), nscr,
                                                          _stream(dev)),
                       name + "_fwd")
        ctx.save_for_backward(s, p, *ws)
        ctx.amp = _lib.current_amp()
        ctx.cfg = (kind, dims, float(p_dropout), float(p_attn_drop), int(seed), bool(recompute))
        ctx.saved_buf = saved
        ctx.in_dtypes = [t.dtype for t in (src, pos, *params)]
        ctx.shapes = (src.shape, pos.shape)
        return out.view(src.shape)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        from .modules import _stream
        s, p, *ws = ctx.saved_tensors
        (name, struct), dims, p_dropout, p_attn_drop, seed, recompute = ctx.cfg
        dev = s.device
        with torch.cuda.device(dev):
            g = f32c(d_out)
            d_src = torch.empty_like(s)
            d_pos = torch.empty_like(p) if ctx.needs_input_grad[1] else None
            grads = grad_buffer(ws, dev)
            nsaved = nbytes(name + "_saved_bytes", *dims)
            nscr = nbytes(name + "_scratch_bytes", *dims, 1)
            _, saved_ptr, scratch = place(dev, nsaved, nscr, recompute, saved=ctx.saved_buf)
            st = _lib.fill(struct, [w.data_ptr() for w in ws])
            gs = _lib.fill(struct, [t.data_ptr() for t in grads])
            with _lib.train_amp(ctx.amp):
                _lib.check(getattr(_lib.lib(), name + "_bwd")(g.data_ptr(), s.data_ptr(), p.data_ptr(), C.byref(st), C.byref(gs),
                                                              d_src.data_ptr(), d_pos.data_ptr() if d_pos is not None else None, *dims,
                                                              p_dropout, p_attn_drop, seed, int(recompute), saved_ptr, nsaved,
                                                              scratch.data_ptr(), nscr, _stream(dev)),
                           name + "_bwd")
        # (the saved activations stay with ctx until autograd releases it: a second backward through the same graph --
        #  retain_graph=True, shared subgraphs -- finds them again)
        d_src, d_pos, *grads = cast([d_src.view(ctx.shapes[0]), d_pos.view(ctx.shapes[1]) if d_pos is not None else None, *grads],
                                    ctx.in_dtypes)
        return (d_src, d_pos, None, None, None, None, None, None, *grads)


def _check_tail(layer) -> None:
    if layer.activation != "relu":
        raise NotImplementedError("axial_vs_amd: only activation='relu' (every shipped config) has a HIP path")
    if abs(layer.norm1.eps - 1e-5) > 0 or abs(layer.norm2.eps - 1e-5) > 0:
        raise NotImplementedError("axial_vs_amd: LayerNorm eps must be 1e-5")


def _apply(layer, src: Tensor, pos: Tensor, kind, dims, dropout: bool, recompute: bool, params: List[Tensor]) -> Tensor:
    p_drop = float(layer.dropout2.p) if dropout else 0.0        # = the attention maps' dropout (reference :164-165) = dropout2 = dropout3
    p_attn = float(layer.dropout1.p) if dropout else 0.0
    return apply(layer, _LayerTrain, src, pos, kind, dims, p_drop, p_attn, draw_seed(layer, p_drop, p_attn), bool(recompute), *params)


def axial_layer_train(layer, src: Tensor, pos: Tensor, dropout: bool = True, recompute: bool = True) -> Tensor:
    """Differentiable forward of a TemporalAxialTrajectoryAttentionLayer through the training tier.
    src [(B T),(H W),C], pos [B,T,H,W,C] -> out like src (fp32).  dropout=False: probabilities forced to 0 (gradients in eval mode)."""
    _check_tail(layer)
    B, T, H, W = pos.shape[:4]
    C_ = src.shape[-1]
    if src.numel() != B * T * H * W * C_ or pos.shape[-1] != C_:
        raise RuntimeError(f"src {tuple(src.shape)} does not match pos {tuple(pos.shape)}")
    dims = (int(B), int(T), int(H), int(W), int(C_), int(layer.n_heads), int(layer.linear1.out_features))
    return _apply(layer, src, pos, _AXIAL, dims, dropout, recompute, layer_parameters(layer))


def traj_layer_train(layer, src: Tensor, pos: Tensor, dropout: bool = True, recompute: bool = True) -> Tensor:
    """Differentiable forward of a TemporalTrajectoryAttentionLayer (the full T*H*W layer, WC/temporal_attention.py:103-155) through
    the training tier: one trajectory attention over all T*H*W tokens of a clip, frames of H*W keys.  src [(B T),(H W),C],
    pos [B,T,H,W,C] -> out like src (fp32).  dropout=False: probabilities forced to 0.  Activations kept: (9 + 3 T) C + d_ffn
    floats per token -- no T*H*W x H*W attention map, which the reference's autograd holds twice."""
    _check_tail(layer)
    B, T, H, W = pos.shape[:4]
    C_ = src.shape[-1]
    if src.numel() != B * T * H * W * C_ or pos.shape[-1] != C_:
        raise RuntimeError(f"src {tuple(src.shape)} does not match pos {tuple(pos.shape)}")
    dims = (int(B), int(T), int(H * W), int(C_), int(layer.n_heads), int(layer.linear1.out_features))
    return _apply(layer, src, pos, _FULL, dims, dropout, recompute, traj_layer_parameters(layer))


# ---- MSDeformAttnTransformerEncoderLayer (WC/msdeformattn.py:177-216): axvs_msda_layer_train_fwd / _bwd ----------------------------------
class _MsdaLayerTrain(torch.autograd.Function):
    """forward / backward of one deformable encoder layer through the library's training tier.  reference_points, the padding
    mask and the spatial shapes are constants (no gradient)."""

    @staticmethod
    def forward(ctx, src, pos, ref, mask, shapes, dims, p_dropout, p_attn_drop, seed, recompute, *params):
        from .modules import _stream
        require_gpu(src)
        s, p, r = f32c(src), f32c(pos), f32c(ref)
        ws = [f32c(w) for w in params]
        dev = s.device
        nsaved = nbytes("axvs_msda_layer_train_saved_bytes", *dims)
        arr = (C.c_int * (2 * len(shapes)))(*[v for hw in shapes for v in hw])
        with torch.cuda.device(dev):
            out = torch.empty_like(s)
            nscr = nbytes("axvs_msda_layer_train_scratch_bytes", *dims, 0)
            saved, saved_ptr, scratch = place(dev, nsaved, nscr, recompute)
            st = _lib.fill(_lib.AxvsMsdaLayerParams, [w.data_ptr() for w in ws])
            _lib.check(_lib.lib().axvs_msda_layer_train_fwd(s.data_ptr(), p.data_ptr() if p is not None else None, r.data_ptr(), r.shape[-1],
                                                            mask.data_ptr() if mask is not None else None, arr, out.data_ptr(), C.byref(st),
                                                            *dims, float(p_dropout), float(p_attn_drop), int(seed), saved_ptr, nsaved,
                                                            scratch.data_ptr(), nscr, _stream(dev)), "axvs_msda_layer_train_fwd")
        ctx.save_for_backward(s, p, r, mask, *ws)
        ctx.amp = _lib.current_amp()
        ctx.cfg = (arr, dims, float(p_dropout), float(p_attn_drop), int(seed), bool(recompute))
        ctx.saved_buf = saved
        ctx.in_dtypes = [t.dtype if t is not None else None for t in (src, pos, *params)]
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        from .modules import _stream
        s, p, r, mask, *ws = ctx.saved_tensors
        arr, dims, p_dropout, p_attn_drop, seed, recompute = ctx.cfg
        dev = s.device
        with torch.cuda.device(dev):
            g = f32c(d_out)
            d_src = torch.empty_like(s)
            d_pos = torch.empty_like(p) if p is not None and ctx.needs_input_grad[1] else None
            grads = grad_buffer(ws, dev)
            nsaved = nbytes("axvs_msda_layer_train_saved_bytes", *dims)
            nscr = nbytes("axvs_msda_layer_train_scratch_bytes", *dims, 1)
            _, saved_ptr, scratch = place(dev, nsaved, nscr, recompute, saved=ctx.saved_buf)
            st = _lib.fill(_lib.AxvsMsdaLayerParams, [w.data_ptr() for w in ws])
            gs = _lib.fill(_lib.AxvsMsdaLayerParams, [t.data_ptr() for t in grads])
            with _lib.train_amp(ctx.amp):
                _lib.check(_lib.lib().axvs_msda_layer_train_bwd(g.data_ptr(), s.data_ptr(), p.data_ptr() if p is not None else None,
                                                                r.data_ptr(), r.shape[-1], mask.data_ptr() if mask is not None else None, arr,
                                                                C.byref(st), C.byref(gs), d_src.data_ptr(),
                                                                d_pos.data_ptr() if d_pos is not None else None, *dims, p_dropout, p_attn_drop,
                                                                seed, int(recompute), saved_ptr, nsaved, scratch.data_ptr(), nscr,
                                                                _stream(dev)), "axvs_msda_layer_train_bwd")
        d_src, d_pos, *grads = cast([d_src, d_pos, *grads], ctx.in_dtypes)
        return (d_src, d_pos, None, None, None, None, None, None, None, None, *grads)


def msda_layer_dims(layer, src: Tensor, shapes) -> tuple:
    a = layer.self_attn
    return (int(src.shape[0]), int(src.shape[1]), int(layer.d_model), int(a.n_heads), int(len(shapes)), int(a.n_points), int(layer.d_ffn))


def msda_layer_train(layer, src: Tensor, pos, reference_points: Tensor, spatial_shapes, padding_mask=None, dropout: bool = True,
                     recompute: bool = False) -> Tensor:
    """Differentiable forward of an MSDeformAttnTransformerEncoderLayer (WC/msdeformattn.py:177-216) through the training tier.
    src [N,S,C]; pos [N,S,C] or None; reference_points [N,S,L,2 | 4] (constants: no gradient); spatial_shapes [(H_l, W_l)]; padding_mask
    [N,S] bool or None -> out like src (fp32).  dropout=False: probabilities forced to 0 (gradients in eval mode).  Dropout sites 7 / 8 / 9
    of include/axvs.h (dropout1 / dropout2 / dropout3), seeded by ``layer.dropout_seed`` or torch's CPU generator."""
    from .msda import _shapes_host
    if layer.norm1.eps != 1e-5 or layer.norm2.eps != 1e-5:
        raise NotImplementedError("axial_vs_amd: LayerNorm eps must be 1e-5")
    if dropout and layer.dropout2.p != layer.dropout3.p:
        raise NotImplementedError("axial_vs_amd: the training tier takes one probability for dropout2 and dropout3")
    shapes = _shapes_host(spatial_shapes)
    if reference_points.requires_grad:
        raise NotImplementedError("axial_vs_amd: reference_points are constants in the training tier (no gradient)")
    if pos is not None and pos.shape != src.shape:
        raise RuntimeError(f"pos {tuple(pos.shape)} does not match src {tuple(src.shape)}")
    if tuple(reference_points.shape[:3]) != (src.shape[0], src.shape[1], len(shapes)):
        raise RuntimeError(f"reference_points {tuple(reference_points.shape)} do not match src {tuple(src.shape)} and {len(shapes)} levels")
    mask = None
    if padding_mask is not None:
        if not padding_mask.is_cuda:
            raise RuntimeError("axial_vs_amd: padding_mask must be a CUDA tensor (no CPU fallback)")
        if tuple(padding_mask.shape) != tuple(src.shape[:2]):
            raise RuntimeError(f"padding_mask {tuple(padding_mask.shape)} does not match src {tuple(src.shape)}")
        mask = padding_mask.to(torch.uint8).contiguous()
    p_drop = float(layer.dropout2.p) if dropout else 0.0
    p_attn = float(layer.dropout1.p) if dropout else 0.0
    return apply(layer, _MsdaLayerTrain, src, pos, reference_points.detach(), mask, shapes, msda_layer_dims(layer, src, shapes), p_drop,
                 p_attn, draw_seed(layer, p_drop, p_attn), bool(recompute), *msda_layer_parameters(layer))
